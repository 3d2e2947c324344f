// The sequencer's host functions (csrc/wire.cpp) and its workspace layout
// (csrc/dvcc_wire_layout.h) under the address and undefined-behaviour
// sanitizers, a program of its own.
//  1. Every prefix length of a valid client mbuf and of a valid ack mbuf, each
//     in a heap block of exactly that length so a read past it is caught, is
//     refused (the full length is taken).
//  2. The sequencer's workspace fields for nb around the scan chunk: aligned to
//     their element types, disjoint, inside the size the same walk reports
//     without a base.  The sizes are stated here on their own.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dvcc_wire_layout.h"

using namespace dvcc;

static void put(std::vector<uint8_t> &b, const void *p, size_t n) {
    const uint8_t *q = static_cast<const uint8_t *>(p);
    b.insert(b.end(), q, q + n);
}
template <class T>
static void put(std::vector<uint8_t> &b, T v) {
    put(b, &v, sizeof(T));
}

static void header(std::vector<uint8_t> &b, uint32_t rtype, uint64_t txn_id, uint64_t batch_id) {
    put<uint32_t>(b, rtype);
    put<uint64_t>(b, txn_id);
    put<uint64_t>(b, batch_id);
    for (int i = 0; i < 8; i++) put<uint64_t>(b, 0);  // mq_time, 7 latencies
}

static std::vector<uint8_t> client_mbuf() {  // two CL_QRYs of 2 and 3 requests from client 3 to node 1
    std::vector<uint8_t> b;
    put<uint32_t>(b, 1), put<uint32_t>(b, 3), put<uint32_t>(b, 2);
    for (uint32_t m = 0; m < 2; m++) {
        header(b, DV_WIRE_CL_QRY, ~0ull, ~0ull);
        put<uint64_t>(b, 77 + m);  // client_startts
        put<uint64_t>(b, 2), put<uint64_t>(b, 0), put<uint64_t>(b, 1);
        put<uint64_t>(b, 2 + m);
        for (uint32_t r = 0; r < 2 + m; r++) {
            put<uint32_t>(b, r & 1), put<uint32_t>(b, 0), put<uint64_t>(b, 10 * m + r), put<uint64_t>(b, 0x5A);
        }
    }
    return b;
}

static std::vector<uint8_t> ack_mbuf() {  // three acks of batch 9 from node 0 to node 1
    std::vector<uint8_t> b;
    put<uint32_t>(b, 1), put<uint32_t>(b, 0), put<uint32_t>(b, 3);
    for (uint32_t m = 0; m < 3; m++) {
        header(b, DV_WIRE_CALVIN_ACK, 1 + 2 * m, 9);
        put<uint32_t>(b, 0);
    }
    return b;
}

static int prefixes() {
    int bad = 0;
    dv_wire_cfg cfg{};
    cfg.workload = DV_YCSB, cfg.calvin = 1, cfg.node_id = 1, cfg.node_cnt = 2, cfg.part_cnt = 2;
    cfg.synth_table_size = 100;
    const std::vector<uint8_t> cm = client_mbuf(), am = ack_mbuf();
    std::vector<uint8_t> out(8192);
    std::vector<uint64_t> boff(64), wst(16);
    std::vector<uint32_t> dfirst(3), wcl(16), wak(16);
    for (size_t len = 0; len <= cm.size(); len++) {
        uint8_t *p = static_cast<uint8_t *>(std::malloc(len ? len : 1));  // (exactly the prefix)
        std::memcpy(p, cm.data(), len);
        const uint64_t off[2] = {0, len};
        dv_wire_seq_in in{p, len, off, 1, 0, 5, 4, 16};
        dv_wire_seq_out o{out.data(), out.size(), boff.data(), 32, 0, dfirst.data(), wcl.data(), wst.data(), wak.data()};
        dv_wire_seq_result r{};
        const int rc = dv_wire_sequence(&cfg, &in, &o, &r);
        const bool whole = len == cm.size();
        if (whole ? (rc != DV_OK || r.n_txn != 2 || r.n_taken != 1 || r.n_msgs != 4) : (rc != DV_ERR_ARG || r.n_taken != 0 || r.n_txn != 0))
            bad |= std::printf("client prefix %zu: rc %d, %u txns\n", len, rc, r.n_txn);
        std::free(p);
    }
    for (size_t len = 0; len <= am.size(); len++) {
        uint8_t *p = static_cast<uint8_t *>(std::malloc(len ? len : 1));
        std::memcpy(p, am.data(), len);
        const uint64_t off[2] = {0, len};
        uint32_t acks[3] = {1, 2, 1};
        const uint32_t client[3] = {2, 3, 2};
        const uint64_t cst[3] = {5, 6, 7};
        dv_wire_seq_ack_in in{p, len, off, 1, 4, 9, 3, 0, client, cst, acks};
        dv_wire_rsp_out o{out.data(), out.size(), boff.data(), 32, 0};
        dv_wire_seq_ack_result r{};
        const int rc = dv_wire_sequence_acks(&cfg, &in, &o, &r);
        const bool whole = len == am.size();
        if (whole ? (rc != DV_OK || r.n_acks != 3 || r.n_done != 2 || acks[1] != 1)
                  : (rc != DV_ERR_ARG || r.first_bad != 0 || acks[0] != 1 || acks[1] != 2 || acks[2] != 1))
            bad |= std::printf("ack prefix %zu: rc %d, first_bad %u\n", len, rc, r.first_bad);
        std::free(p);
    }
    return bad;
}

struct Field {
    const char *name;
    const void *p;
    uint64_t bytes, align;
};
template <class T>
static Field field(const char *name, const T *p, uint64_t n) {
    return Field{name, p, n * sizeof(T), alignof(T)};
}

static int layout(uint32_t nb, uint32_t nodes, uint32_t max_txn) {
    int bad = 0;
    const uint64_t n = nb ? nb : 1, nc = (n + kWireChunk - 1) / kWireChunk;
    // a list entry per (txn, participant) and two more per destination; a tile entry per kSeqTile list entries
    const uint64_t per_mbuf = std::min<uint64_t>((4096 - 12) / 24, 40ull * nodes);
    const uint64_t nl = std::min<uint64_t>(n * per_mbuf, (uint64_t)max_txn * std::min(nodes, 128u)) + 2ull * nodes;
    const uint64_t ntile = (std::min<uint64_t>(n * 40, max_txn) + 1 + 255) / 256;
    WireSeqWs w;
    const uint64_t bytes = wire_seq_ws_layout(nullptr, nb, nodes, max_txn, w);
    std::vector<uint64_t> mem(bytes / 8 + 1);
    char *base = reinterpret_cast<char *>(mem.data());
    if (wire_seq_ws_layout(base, nb, nodes, max_txn, w) != bytes) bad |= std::printf("nb=%u: two sizes\n", nb);
    const std::vector<Field> fs = {
        {"res", w.res, kWireResBytes, 8}, field("first", w.first, 2), field("moff", w.moff, n * 40), field("bt", w.bt, n),
        field("ba", w.ba, n), field("bm", w.bm, n), field("ct", w.ct, nc), field("ca", w.ca, nc), field("cm", w.cm, nc),
        {"plan", w.plan, sizeof(WireSeqPlan), 4}, field("mmask", w.mmask, n * 40), field("msz", w.msz, n * 40),
        field("dcnt", w.dcnt, n * nodes), field("dbyt", w.dbyt, n * nodes), field("dtot", w.dtot, nodes),
        field("dtotb", w.dtotb, nodes), field("dmb", w.dmb, nodes), field("dMB", w.dMB, nodes), field("dDB", w.dDB, nodes),
        field("lS", w.lS, nl), field("ljmp", w.ljmp, nl), field("lpos", w.lpos, nl), field("tent", w.tent, ntile * nodes),
        field("tmb", w.tmb, ntile * nodes)};
    for (const Field &f : fs) {
        const char *p = static_cast<const char *>(f.p);
        if (p < base || reinterpret_cast<uintptr_t>(p) % f.align || p + f.bytes > base + bytes)
            bad |= std::printf("nb=%u nodes=%u: %s misaligned or outside its %llu bytes\n", nb, nodes, f.name, (unsigned long long)bytes);
        for (const Field &g : fs) {
            const char *q = static_cast<const char *>(g.p);
            if (&f != &g && p < q + g.bytes && q < p + f.bytes) bad |= std::printf("nb=%u: %s overlaps %s\n", nb, f.name, g.name);
        }
    }
    if (static_cast<const void *>(w.sres) != w.res) bad |= std::printf("nb=%u: sres is not res\n", nb);
    return bad;
}

int main() {
    int bad = prefixes(), n = 0;
    for (uint32_t nb : {0u, 1u, 2u, kWireChunk - 1, kWireChunk, kWireChunk + 1, 2 * kWireChunk + 1})
        for (uint32_t nodes : {1u, 5u, 64u})
            for (uint32_t max_txn : {1u, 1000u, 1u << 20}) bad |= layout(nb, nodes, max_txn), n++;
    if (!bad) std::printf("ok %d\n", n);
    return bad ? 1 : 0;
}
