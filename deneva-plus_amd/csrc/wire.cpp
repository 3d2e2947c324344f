// wire.cpp -- Deneva's message batches in and out of the engine's host epochs.
//
// Ingress: a batch as runcl's MessageThread sends it (transport/msg_thread.cpp:
// 53-111, mbuf in msg_thread.h:24-62) is decoded message by message straight
// into the epoch's host arrays -- what Message::create_messages (message.cpp:
// 29-50) + copy_from_buf (YCSB 493-510, TPC-C 620-655, ClientQueryMessage
// 889-903, Message header 224-246) + the txn managers' access lists do, without
// a Message object or a per-request allocation.  Egress: the epoch's outcome
// as the replies the reference's server sends (CL_RSP, worker_thread.cpp:152;
// CALVIN_ACK, 127-136), packed into mbufs the same way.
//
// Byte layout (COPY_VAL / COPY_BUF, system/helper.h:155-169: memcpy of
// sizeof(field), fields back to back, no alignment): see include/dvcc.h.  The
// reader below never dereferences a field in place (memcpy out of the byte
// stream), so unaligned offsets are fine.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dvcc.h"

namespace {

constexpr uint64_t kU64Max = ~0ull;
constexpr uint32_t kMaxReq = 128;   // the engine's longest txn (kMaxPos)
constexpr uint64_t kYcsbReq = 24;   // sizeof(ycsb_request) on x86-64

// Message::mget_size (message.cpp:196-209): rtype, txn_id, [batch_id], mq_time, 7 doubles
uint64_t hdr_size(const dv_wire_cfg *c) { return 4 + 8 + (c->calvin ? 8 : 0) + 8 + 7 * 8; }

struct Reader {  // bounds-checked COPY_VAL over [p, end)
    const uint8_t *p, *end;
    bool ok = true;
    template <class T>
    T get() {
        T v{};
        if ((uint64_t)(end - p) < sizeof(T)) {
            ok = false;
            p = end;
            return v;
        }
        std::memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
    void skip(uint64_t n) {
        if ((uint64_t)(end - p) < n) {
            ok = false;
            p = end;
        } else {
            p += n;
        }
    }
};

struct Writer {  // COPY_BUF into [p, end)
    uint8_t *p;
    template <class T>
    void put(const T &v) {
        std::memcpy(p, &v, sizeof(T));
        p += sizeof(T);
    }
    void zeros(uint64_t n) {
        std::memset(p, 0, n);
        p += n;
    }
};

// one decoded message, checked, before it touches the epoch
struct Msg {
    uint32_t rtype = 0;
    uint64_t txn_id = kU64Max, batch_id = kU64Max, client_startts = 0;
    uint32_t n_acc = 0;
    const uint8_t *reqs = nullptr;  // YCSB: the request records
    dv_tpcc_query tq;               // TPC-C
};

// Message header + ClientQueryMessage part; false if malformed
bool read_client_part(const dv_wire_cfg *c, Reader &r, Msg &m, bool check) {
    m.rtype = r.get<uint32_t>();
    m.txn_id = r.get<uint64_t>();
    if (c->calvin) m.batch_id = r.get<uint64_t>();
    r.skip(8 + 7 * 8);  // mq_time, latency doubles (statistics)
    if (m.rtype == DV_WIRE_RDONE) return r.ok;
    if (m.rtype != DV_WIRE_CL_QRY) return false;  // (clients and sequencers send CL_QRY)
    m.client_startts = r.get<uint64_t>();
    const uint64_t np = r.get<uint64_t>();  // size_t partitions
    if (!r.ok || np > DV_TPCC_MAX_PARTS) return false;
    if (!check) {
        r.skip(np * 8);
        return r.ok;
    }
    for (uint64_t i = 0; i < np; i++) {
        const uint64_t part = r.get<uint64_t>();
        if (part >= c->part_cnt) return false;
    }
    return r.ok;
}

bool read_ycsb(const dv_wire_cfg *c, Reader &r, Msg &m, bool check) {
    const uint64_t n = r.get<uint64_t>();  // size_t requests
    const uint32_t lim = std::min<uint32_t>(c->max_req ? c->max_req : kMaxReq, kMaxReq);
    if (!r.ok || n > lim || (uint64_t)(r.end - r.p) < n * kYcsbReq) return false;
    m.reqs = r.p;
    m.n_acc = (uint32_t)n;
    for (uint64_t i = 0; check && i < n; i++) {
        uint32_t acctype;
        uint64_t key;
        std::memcpy(&acctype, r.p + i * kYcsbReq, 4);
        std::memcpy(&key, r.p + i * kYcsbReq + 8, 8);
        if (acctype > DV_WR || key >= c->synth_table_size) return false;  // RD / WR; assert(key < g_synth_table_size)
    }
    r.skip(n * kYcsbReq);
    return r.ok;
}

bool read_tpcc(Reader &r, Msg &m) {
    dv_tpcc_query &q = m.tq;
    std::memset(&q, 0, sizeof(q));
    q.txn_type = r.get<uint64_t>();
    q.w_id = r.get<uint64_t>();
    q.d_id = r.get<uint64_t>();
    q.c_id = r.get<uint64_t>();
    q.d_w_id = r.get<uint64_t>();
    q.c_w_id = r.get<uint64_t>();
    q.c_d_id = r.get<uint64_t>();
    for (char &ch : q.c_last) ch = (char)r.get<uint8_t>();
    q.h_amount = r.get<uint64_t>();
    q.by_last_name = r.get<uint8_t>() != 0;
    const uint64_t n = r.get<uint64_t>();  // size_t items
    if (!r.ok || n > DV_TPCC_MAX_OL) return false;
    for (uint64_t i = 0; i < n; i++) {
        q.items[i].ol_i_id = r.get<uint64_t>();
        q.items[i].ol_supply_w_id = r.get<uint64_t>();
        q.items[i].ol_quantity = r.get<uint64_t>();
    }
    q.rbk = r.get<uint8_t>() != 0;
    q.remote = r.get<uint8_t>() != 0;
    q.ol_cnt = r.get<uint64_t>();
    q.o_entry_d = r.get<uint64_t>();
    if (!r.ok) return false;
    // the txn manager walks items[0 .. ol_cnt) (new_order_6..9): the list must hold them
    if (q.txn_type == 2 && q.ol_cnt != n) return false;
    if (q.txn_type == 1) q.ol_cnt = 0;  // (a Payment carries no items)
    if (q.txn_type != 1 && q.txn_type != 2) return false;
    m.n_acc = q.txn_type == 1 ? 3 : (uint32_t)(3 + 2 * q.ol_cnt);
    return true;
}

}  // namespace

extern "C" int dv_wire_epoch_reset(dv_wire_epoch *ep) {
    if (!ep || !ep->txn_begin) return DV_ERR_ARG;
    ep->n_txn = 0;
    ep->n_acc = 0;
    ep->rdone = 0;
    ep->batch_id = kU64Max;
    ep->txn_begin[0] = 0;
    return DV_OK;
}

namespace {
// a parsed TPC-C query's fields as the access-list expansion checks them (into scratch arrays)
bool tpcc_fields_ok(const dv_wire_cfg *c, const Msg &m) {
    uint64_t k[3 + 2 * DV_TPCC_MAX_OL], a[3 + 2 * DV_TPCC_MAX_OL];
    uint8_t ty[3 + 2 * DV_TPCC_MAX_OL], tb[3 + 2 * DV_TPCC_MAX_OL];
    uint32_t beg[2];
    return dv_tpcc_expand(c->tpcc, &m.tq, 1, 3 + 2 * DV_TPCC_MAX_OL, k, ty, tb, a, beg, nullptr, nullptr) == DV_OK;
}

// one message at r: header, client part and body, every field checked (the
// TPC-C ones by the access-list expansion into scratch arrays) -- or, for a
// batch dv_wire_open has checked (check false), only parsed
bool read_msg(const dv_wire_cfg *c, Reader &r, Msg &m, bool check = true) {
    if (!read_client_part(c, r, m, check)) return false;
    if (c->calvin ? m.batch_id == kU64Max : m.rtype == DV_WIRE_RDONE) return false;  // (RDONE ends Calvin batches)
    if (m.rtype == DV_WIRE_RDONE) return true;
    if (c->workload != DV_TPCC) return read_ycsb(c, r, m, check);
    if (!read_tpcc(r, m)) return false;
    return !check || tpcc_fields_ok(c, m);
}

bool cfg_ok(const dv_wire_cfg *c) {
    return c && c->part_cnt && c->node_cnt && (c->workload == DV_YCSB || (c->workload == DV_TPCC && c->tpcc));
}
}  // namespace

extern "C" int dv_wire_open(const dv_wire_cfg *cfg, const uint8_t *batch, uint64_t len, dv_wire_cursor *cur) {
    if (!cfg_ok(cfg) || !cur || !batch || len < DV_WIRE_HDR || len > DV_WIRE_MSG_MAX) return DV_ERR_ARG;
    uint32_t h[3];
    std::memcpy(h, batch, sizeof(h));
    // create_messages' asserts (message.cpp:39-41): addressed here, from another node, not empty
    if (h[0] != cfg->node_id || h[1] == cfg->node_id || h[2] == 0) return DV_ERR_ARG;
    // the whole batch, message by message, before any of it is decoded:
    // exactly `count` well-formed messages filling exactly `len` bytes
    Reader r{batch + DV_WIRE_HDR, batch + len};
    Msg m;
    for (uint32_t i = 0; i < h[2]; i++)
        if (!read_msg(cfg, r, m)) return DV_ERR_ARG;
    if (r.p != batch + len) return DV_ERR_ARG;
    cur->buf = batch;
    cur->len = len;
    cur->off = DV_WIRE_HDR;
    cur->left = h[2];
    cur->src = h[1];
    return DV_OK;
}

extern "C" int dv_wire_decode(const dv_wire_cfg *cfg, dv_wire_cursor *cur, dv_wire_epoch *ep) {
    if (!cfg_ok(cfg) || !cur || !ep || !cur->buf || !ep->keys || !ep->types || !ep->txn_begin) return DV_ERR_ARG;
    const bool tpcc = cfg->workload == DV_TPCC;
    if (tpcc && (!ep->tables || !ep->args)) return DV_ERR_ARG;
    Msg m;
    while (cur->left > 0) {
        Reader r{cur->buf + cur->off, cur->buf + cur->len};
        if (!read_msg(cfg, r, m, false)) return DV_ERR_ARG;  // (checked whole by dv_wire_open)
        if (cfg->calvin && ep->batch_id != kU64Max) {  // the sequencer's batch (sequencer.cpp:207-210)
            if (m.batch_id < ep->batch_id) return DV_ERR_ARG;  // stale
            if (m.batch_id > ep->batch_id) return DV_WIRE_MORE;
        }
        if (m.rtype == DV_WIRE_RDONE) {
            ep->batch_id = m.batch_id;
            ep->rdone++;
        } else {
            if (ep->n_txn >= ep->max_txn || ep->n_acc + m.n_acc > ep->max_acc) {
                if (ep->n_txn == 0) return DV_ERR_ARG;  // (it would never fit)
                return DV_WIRE_MORE;
            }
            const uint32_t t = ep->n_txn;
            const uint64_t a0 = ep->n_acc;
            if (tpcc) {
                // the access list of TPCCTxnManager (fields checked at dv_wire_open)
                const int rc = dv_tpcc_expand(cfg->tpcc, &m.tq, 1, ep->max_acc - a0, ep->keys + a0, ep->types + a0,
                                              ep->tables + a0, ep->args + a0, ep->txn_begin + t,
                                              ep->txn_type ? ep->txn_type + t : nullptr,
                                              ep->owner ? ep->owner + a0 : nullptr);
                ep->txn_begin[t] = (uint32_t)a0;  // (expand numbered from 0)
                if (rc) return DV_ERR_ARG;
            } else {
                for (uint32_t i = 0; i < m.n_acc; i++) {
                    uint32_t acctype;
                    uint64_t key;
                    std::memcpy(&acctype, m.reqs + i * kYcsbReq, 4);
                    std::memcpy(&key, m.reqs + i * kYcsbReq + 8, 8);
                    ep->keys[a0 + i] = key;
                    ep->types[a0 + i] = (uint8_t)acctype;
                    if (ep->owner) ep->owner[a0 + i] = (uint8_t)(key % cfg->part_cnt);  // key_to_part
                }
                if (ep->tables) std::memset(ep->tables + a0, 0, m.n_acc);
            }
            if (cfg->calvin) ep->batch_id = m.batch_id;
            if (ep->txn_id)  // Calvin: the sequencer's id; else WorkerThread::get_next_txn_id for one worker
                ep->txn_id[t] = cfg->calvin ? m.txn_id : cfg->node_id + (uint64_t)cfg->node_cnt * ep->next_txn;
            if (!cfg->calvin) ep->next_txn++;
            if (ep->client_startts) ep->client_startts[t] = m.client_startts;
            if (ep->return_node) ep->return_node[t] = cur->src;
            ep->n_acc = a0 + m.n_acc;
            ep->n_txn = t + 1;
            ep->txn_begin[t + 1] = (uint32_t)ep->n_acc;
        }
        cur->off = (uint64_t)(r.p - cur->buf);
        cur->left--;
    }
    return DV_OK;
}

extern "C" int dv_wire_decode_batches(const dv_wire_cfg *cfg, const uint8_t *buf, const uint64_t *off,
                                      uint32_t n_batches, dv_wire_cursor *cur, uint32_t *next_batch,
                                      dv_wire_epoch *ep) {
    if (!cfg || !buf || !off || !cur || !next_batch || !ep) return DV_ERR_ARG;
    for (;;) {
        if (cur->buf && cur->left > 0) {
            const int rc = dv_wire_decode(cfg, cur, ep);
            if (rc) return rc;  // DV_WIRE_MORE (the cursor holds the rest) or an error
        }
        if (*next_batch >= n_batches) return DV_OK;
        const uint32_t b = *next_batch;
        if (off[b + 1] < off[b]) return DV_ERR_ARG;
        const int rc = dv_wire_open(cfg, buf + off[b], off[b + 1] - off[b], cur);
        if (rc) return rc;  // (*next_batch stays at the refused batch)
        *next_batch = b + 1;
    }
}

extern "C" int dv_wire_respond(const dv_wire_cfg *cfg, const dv_wire_epoch *ep, const uint8_t *commit, uint8_t *out,
                               uint64_t cap, uint64_t *batch_off, uint32_t max_batches, uint32_t *n_batches) {
    if (!cfg || !ep || !out || !batch_off || !n_batches || !ep->txn_id || !ep->return_node) return DV_ERR_ARG;
    if (!cfg->calvin && (!commit || !ep->client_startts)) return DV_ERR_ARG;
    const uint64_t H = hdr_size(cfg);
    // ClientResponseMessage: header + client_startts; AckMessage: header + RC (4 bytes)
    const uint64_t msz = cfg->calvin ? H + 4 : H + 8;
    std::vector<uint32_t> order;
    order.reserve(ep->n_txn);
    for (uint32_t t = 0; t < ep->n_txn; t++)
        if (cfg->calvin || commit[t]) order.push_back(t);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return ep->return_node[a] < ep->return_node[b]; });
    const uint32_t per = (uint32_t)((DV_WIRE_MSG_MAX - DV_WIRE_HDR) / msz);
    uint64_t pos = 0;
    uint32_t nb = 0;
    size_t i = 0;
    batch_off[0] = 0;
    while (i < order.size()) {
        const uint32_t dest = ep->return_node[order[i]];
        size_t j = i;
        while (j < order.size() && j - i < per && ep->return_node[order[j]] == dest) j++;
        const uint64_t bytes = DV_WIRE_HDR + (j - i) * msz;
        if (nb >= max_batches || pos + bytes > cap) return DV_ERR_ARG;
        Writer w{out + pos};
        w.put<uint32_t>(dest);
        w.put<uint32_t>(cfg->node_id);
        w.put<uint32_t>((uint32_t)(j - i));
        for (size_t k = i; k < j; k++) {
            const uint32_t t = order[k];
            w.put<uint32_t>(cfg->calvin ? DV_WIRE_CALVIN_ACK : DV_WIRE_CL_RSP);
            w.put<uint64_t>(ep->txn_id[t]);
            if (cfg->calvin) w.put<uint64_t>(ep->batch_id);
            w.zeros(8 + 7 * 8);  // mq_time, latencies
            if (cfg->calvin)
                w.put<uint32_t>(0);  // RC RCOK: a Calvin txn's rc at calvin_wrapup (txn.cpp:287)
            else
                w.put<uint64_t>(ep->client_startts[t]);
        }
        pos += bytes;
        batch_off[++nb] = pos;
        i = j;
    }
    *n_batches = nb;
    return DV_OK;
}

// ---- the CALVIN sequencer (system/sequencer.cpp) on the host: the yardstick
// of dv_wire_sequence_device / dv_wire_sequence_acks_device (dvcc_wire.hip).
namespace {

constexpr uint64_t kSeqHdr = 84;          // a CALVIN build's Message header
constexpr uint64_t kAckBytes = 88;        // AckMessage: header + RC
constexpr uint64_t kSeqRspBytes = 92;     // ClientResponseMessage: header + client_startts
constexpr uint32_t kAckPer = (DV_WIRE_MSG_MAX - DV_WIRE_HDR) / kAckBytes;  // 46

// the knobs themselves, as the expansion of no query checks them
bool tpcc_knobs_ok(const dv_tpcc_params *tp) {
    uint64_t k, a;
    uint8_t ty, tb;
    uint32_t beg;
    return tp && dv_tpcc_expand(tp, nullptr, 0, 0, &k, &ty, &tb, &a, &beg, nullptr, nullptr) == DV_OK;
}

bool seq_cfg_ok(const dv_wire_cfg *c) {
    return c && (c->workload == DV_YCSB || (c->workload == DV_TPCC && tpcc_knobs_ok(c->tpcc))) && c->calvin == 1 &&
           c->part_cnt && c->node_cnt && c->node_cnt <= DV_WIRE_SEQ_NODE_MAX && c->node_id < c->node_cnt;
}

// mbuf b of the queue: its bytes, false where off decreases, points past the
// buffer, or the length is outside [12, 4096]
bool seq_span(const uint64_t *off, uint32_t b, uint64_t buf_len, uint64_t &o0, uint64_t &len) {
    o0 = off[b];
    const uint64_t o1 = off[b + 1];
    if (o1 < o0 || o1 > buf_len || o1 - o0 < DV_WIRE_HDR || o1 - o0 > DV_WIRE_MSG_MAX) return false;
    len = o1 - o0;
    return true;
}

struct SeqTxn {
    const uint8_t *msg;  // the client's message
    uint32_t len, src;
    uint64_t cst, parts;
};

// a client mbuf's txns appended to `txns`; false (and nothing appended) where it is malformed
bool seq_client_mbuf(const dv_wire_cfg *cfg, uint32_t n_dest, const uint8_t *p, uint64_t len,
                     std::vector<SeqTxn> &txns) {
    uint32_t h[3];
    std::memcpy(h, p, sizeof(h));
    if (h[0] != cfg->node_id || h[1] < cfg->node_cnt || h[1] >= n_dest || h[2] == 0) return false;
    const size_t keep = txns.size();
    Reader r{p + DV_WIRE_HDR, p + len};
    for (uint32_t i = 0; i < h[2]; i++) {
        Msg m;
        const uint8_t *at = r.p;
        // (the message's own txn_id and batch_id are not looked at: a client sends UINT64_MAX in both)
        bool ok = read_client_part(cfg, r, m, true) && m.rtype == DV_WIRE_CL_QRY;
        if (ok && cfg->workload == DV_TPCC)
            ok = read_tpcc(r, m) && tpcc_fields_ok(cfg, m);
        else if (ok)
            ok = read_ycsb(cfg, r, m, true) && m.n_acc > 0;
        if (!ok) {
            txns.resize(keep);
            return false;
        }
        uint64_t parts = 0;
        if (cfg->workload == DV_TPCC) {
            // TPCCQuery::participants: GET_NODE_ID(wh_to_part(w)) of w_id and, for a Payment, c_w_id, for a
            // NewOrder, its items' supply warehouses (read_tpcc: a Payment's ol_cnt is 0, its items never count)
            const auto node = [&](uint64_t w) { return ((w - 1) % cfg->tpcc->part_cnt) % cfg->node_cnt; };
            parts |= 1ull << node(m.tq.w_id);
            if (m.tq.txn_type == 1) parts |= 1ull << node(m.tq.c_w_id);
            for (uint64_t q = 0; q < m.tq.ol_cnt; q++) parts |= 1ull << node(m.tq.items[q].ol_supply_w_id);
        } else {  // YCSBQuery::participants: GET_NODE_ID(key_to_part(key))
            for (uint32_t q = 0; q < m.n_acc; q++) {
                uint64_t key;
                std::memcpy(&key, m.reqs + q * kYcsbReq + 8, 8);
                parts |= 1ull << ((key % cfg->part_cnt) % cfg->node_cnt);
            }
        }
        txns.push_back(SeqTxn{at, (uint32_t)(r.p - at), h[1], m.client_startts, parts});
    }
    if (r.p != p + len) {
        txns.resize(keep);
        return false;
    }
    return true;
}

}  // namespace

extern "C" int dv_wire_sequence(const dv_wire_cfg *cfg, const dv_wire_seq_in *in, const dv_wire_seq_out *out,
                                dv_wire_seq_result *res) {
    if (!seq_cfg_ok(cfg) || !in || !out || !res || !in->buf || !in->off) return DV_ERR_ARG;
    if (!out->out || !out->batch_off || !out->dest_first || !out->wait_client || !out->wait_startts || !out->wait_acks)
        return DV_ERR_ARG;
    if (in->batch_id == kU64Max || !in->max_txn || in->first_batch > in->n_batches) return DV_ERR_ARG;
    if (in->n_dest < cfg->node_cnt || in->n_dest > DV_WIRE_DEST_MAX) return DV_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(out->out) & 3u) return DV_ERR_ARG;
    // the mbufs taken
    std::vector<SeqTxn> txns;
    int status = DV_OK;
    uint32_t b = in->first_batch;
    for (; b < in->n_batches; b++) {
        uint64_t o0, len;
        const size_t before = txns.size();
        if (!seq_span(in->off, b, in->buf_len, o0, len) || !seq_client_mbuf(cfg, in->n_dest, in->buf + o0, len, txns)) {
            status = DV_ERR_ARG;
            break;
        }
        if (txns.size() > in->max_txn) {
            txns.resize(before);
            status = b == in->first_batch ? DV_ERR_ARG : DV_WIRE_MORE;
            break;
        }
    }
    // every destination's mbufs: MessageThread::run's greedy cut over its messages and the RDONE
    const uint32_t nodes = cfg->node_cnt;
    struct Mbuf { uint32_t dest, first, count; uint64_t at; };  // its messages: the destination's [first, first + count)
    std::vector<std::vector<uint32_t>> list(nodes);             // a destination's txns
    std::vector<Mbuf> mb;
    uint64_t pos = 0, n_msgs = 0;
    for (uint32_t k = 0; k < txns.size(); k++)
        for (uint32_t d = 0; d < nodes; d++)
            if (txns[k].parts >> d & 1) list[d].push_back(k), n_msgs++;
    std::vector<uint32_t> dest_first(nodes + 1);
    for (uint32_t d = 0; d < nodes; d++) {
        dest_first[d] = (uint32_t)mb.size();
        const uint32_t n = (uint32_t)list[d].size();
        uint64_t size = DV_WIRE_MSG_MAX + 1;  // (no mbuf open)
        for (uint32_t i = 0; i <= n; i++) {   // (i == n: the RDONE)
            const uint64_t len = i < n ? txns[list[d][i]].len : kSeqHdr;
            if (size + len > DV_WIRE_MSG_MAX) {
                mb.push_back(Mbuf{d, i, 0, pos});
                size = DV_WIRE_HDR;
                pos += DV_WIRE_HDR;
            }
            mb.back().count++;
            size += len;
            pos += len;
        }
    }
    dest_first[nodes] = (uint32_t)mb.size();
    res->n_taken = b;
    res->n_txn = (uint32_t)txns.size();
    res->n_out = (uint32_t)mb.size();
    res->n_msgs = n_msgs;
    res->n_bytes = pos;
    if (pos > out->cap || mb.size() > out->max_batches) return res->status = DV_ERR_ARG;  // (nothing written)
    res->status = status;
    for (uint32_t k = 0; k < txns.size(); k++) {
        out->wait_client[k] = txns[k].src;
        out->wait_startts[k] = txns[k].cst;
        out->wait_acks[k] = (uint32_t)__builtin_popcountll(txns[k].parts);
    }
    std::memcpy(out->dest_first, dest_first.data(), dest_first.size() * sizeof(uint32_t));
    for (size_t j = 0; j < mb.size(); j++) {
        const Mbuf &m = mb[j];
        out->batch_off[j] = m.at;
        Writer w{out->out + m.at};
        w.put<uint32_t>(m.dest);
        w.put<uint32_t>(cfg->node_id);
        w.put<uint32_t>(m.count);
        for (uint32_t i = m.first; i < m.first + m.count; i++) {
            const bool done = i == list[m.dest].size();
            const uint32_t k = done ? 0 : list[m.dest][i];
            w.put<uint32_t>(done ? DV_WIRE_RDONE : DV_WIRE_CL_QRY);
            w.put<uint64_t>(done ? kU64Max : cfg->node_id + (uint64_t)nodes * k);
            w.put<uint64_t>(in->batch_id);
            w.zeros(8 + 7 * 8);  // mq_time, latencies
            if (!done) {
                std::memcpy(w.p, txns[k].msg + kSeqHdr, txns[k].len - kSeqHdr);
                w.p += txns[k].len - kSeqHdr;
            }
        }
    }
    out->batch_off[mb.size()] = pos;
    return status;
}

extern "C" int dv_wire_sequence_acks(const dv_wire_cfg *cfg, const dv_wire_seq_ack_in *in, const dv_wire_rsp_out *out,
                                     dv_wire_seq_ack_result *res) {
    if (!seq_cfg_ok(cfg) || !in || !out || !res || !in->buf || !in->off || !out->out || !out->batch_off)
        return DV_ERR_ARG;
    if (in->n_txn && (!in->wait_client || !in->wait_startts || !in->wait_acks)) return DV_ERR_ARG;
    if (in->batch_id == kU64Max || !in->n_dest || in->n_dest > DV_WIRE_DEST_MAX) return DV_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(out->out) & 3u) return DV_ERR_ARG;
    *res = dv_wire_seq_ack_result{DV_ERR_ARG, DV_WIRE_NO_BATCH, 0, 0, 0, 0, 0};
    // per txn: its acks in the call and the position of the last
    std::vector<uint32_t> cnt(in->n_txn, 0);
    std::vector<uint64_t> last(in->n_txn, 0);
    uint64_t at = 0;  // the stream position: mbuf-major, message-minor
    for (uint32_t b = 0; b < in->n_batches; b++) {
        uint64_t o0, len;
        bool ok = seq_span(in->off, b, in->buf_len, o0, len);
        uint32_t h[3] = {0, 0, 0};
        if (ok) {
            std::memcpy(h, in->buf + o0, sizeof(h));
            ok = h[0] == cfg->node_id && h[1] < cfg->node_cnt && h[2] >= 1 && h[2] <= kAckPer &&
                 len == DV_WIRE_HDR + kAckBytes * h[2];
        }
        for (uint32_t m = 0; ok && m < h[2]; m++, at++) {
            const uint8_t *p = in->buf + o0 + DV_WIRE_HDR + m * kAckBytes;
            uint32_t rtype;
            uint64_t txn_id, bid;
            std::memcpy(&rtype, p, 4);
            std::memcpy(&txn_id, p + 4, 8);
            std::memcpy(&bid, p + 12, 8);
            if (rtype != DV_WIRE_CALVIN_ACK || bid == kU64Max) {
                ok = false;
            } else if (bid != in->batch_id) {
                res->n_skipped++;
            } else if (txn_id % cfg->node_cnt != cfg->node_id || txn_id / cfg->node_cnt >= in->n_txn) {
                ok = false;
            } else {
                const uint64_t k = txn_id / cfg->node_cnt;
                cnt[k]++;
                last[k] = at;
                res->n_acks++;
            }
        }
        if (!ok) {
            *res = dv_wire_seq_ack_result{DV_ERR_ARG, b, 0, 0, 0, 0, 0};
            return DV_ERR_ARG;
        }
    }
    // (a refused call reports no count, but for replies that do not fit)
    const auto refuse = [&] {
        *res = dv_wire_seq_ack_result{DV_ERR_ARG, DV_WIRE_NO_BATCH, 0, 0, 0, 0, 0};
        return DV_ERR_ARG;
    };
    // the txns that complete, in the order of their last acks
    std::vector<uint32_t> done;
    for (uint32_t k = 0; k < in->n_txn; k++) {
        if (cnt[k] > in->wait_acks[k]) return refuse();  // assert(server_ack_cnt > 0)
        if (cnt[k] && cnt[k] == in->wait_acks[k]) {
            if (in->wait_client[k] >= in->n_dest) return refuse();
            done.push_back(k);
        }
    }
    std::sort(done.begin(), done.end(), [&](uint32_t a, uint32_t c) { return last[a] < last[c]; });
    std::stable_sort(done.begin(), done.end(),
                     [&](uint32_t a, uint32_t c) { return in->wait_client[a] < in->wait_client[c]; });
    // dv_wire_respond's packing of 92-byte CL_RSPs, decided before anything is written
    const uint32_t per = (uint32_t)((DV_WIRE_MSG_MAX - DV_WIRE_HDR) / kSeqRspBytes);
    uint32_t nb = 0;
    for (size_t i = 0, j; i < done.size(); i = j, nb++)
        for (j = i; j < done.size() && j - i < per && in->wait_client[done[j]] == in->wait_client[done[i]];) j++;
    res->n_done = (uint32_t)done.size();
    res->n_batches = nb;
    res->n_bytes = (uint64_t)nb * DV_WIRE_HDR + done.size() * kSeqRspBytes;
    if (res->n_bytes > out->cap || nb > out->max_batches) return DV_ERR_ARG;
    for (uint32_t k = 0; k < in->n_txn; k++) in->wait_acks[k] -= cnt[k];
    uint64_t pos = 0;
    nb = 0;
    out->batch_off[0] = 0;
    for (size_t i = 0, j; i < done.size(); i = j) {
        const uint32_t dest = in->wait_client[done[i]];
        for (j = i; j < done.size() && j - i < per && in->wait_client[done[j]] == dest;) j++;
        Writer w{out->out + pos};
        w.put<uint32_t>(dest);
        w.put<uint32_t>(cfg->node_id);
        w.put<uint32_t>((uint32_t)(j - i));
        for (size_t q = i; q < j; q++) {
            w.put<uint32_t>(DV_WIRE_CL_RSP);
            w.put<uint64_t>(cfg->node_id + (uint64_t)cfg->node_cnt * done[q]);
            w.put<uint64_t>(kU64Max);  // batch_id (message.cpp:99-103, 178)
            w.zeros(8 + 7 * 8);
            w.put<uint64_t>(in->wait_startts[done[q]]);
        }
        pos += DV_WIRE_HDR + (j - i) * kSeqRspBytes;
        out->batch_off[++nb] = pos;
    }
    res->status = DV_OK;
    return DV_OK;
}
