// dv_wire_sequence (csrc/wire.cpp) under a TPC-C cfg and the address and
// undefined-behaviour sanitizers, a program of its own.  Every prefix length
// of a valid TPC-C client mbuf -- a Payment and a 62-item NewOrder -- each in
// a heap block of exactly that length so a read past it is caught, is refused
// (the full length is taken, both txns fanned out to their participants).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dvcc.h"

static void put(std::vector<uint8_t> &b, const void *p, size_t n) {
    const uint8_t *q = static_cast<const uint8_t *>(p);
    b.insert(b.end(), q, q + n);
}
template <class T>
static void put(std::vector<uint8_t> &b, T v) {
    put(b, &v, sizeof(T));
}

// a client's CL_QRY of a CALVIN build up to its body: header, client_startts, one partition
static void query_head(std::vector<uint8_t> &b, uint64_t cst) {
    put<uint32_t>(b, DV_WIRE_CL_QRY);
    put<uint64_t>(b, ~0ull), put<uint64_t>(b, ~0ull);  // txn_id, batch_id
    for (int i = 0; i < 8; i++) put<uint64_t>(b, 0);    // mq_time, 7 latencies
    put<uint64_t>(b, cst);
    put<uint64_t>(b, 1), put<uint64_t>(b, 0);
}

static std::vector<uint8_t> client_mbuf() {  // from client 3 to node 1 of two; 4 warehouses on 2 partitions
    std::vector<uint8_t> b;
    put<uint32_t>(b, 1), put<uint32_t>(b, 3), put<uint32_t>(b, 2);
    query_head(b, 77);  // a Payment at warehouse 1 (node 0), its customer at warehouse 2 (node 1)
    for (uint64_t v : {1, 1, 3, 7, 1, 2, 4}) put<uint64_t>(b, v);
    for (int i = 0; i < 16; i++) put<uint8_t>(b, 0);
    put<uint64_t>(b, 500), put<uint8_t>(b, 0), put<uint64_t>(b, 0);
    put<uint8_t>(b, 0), put<uint8_t>(b, 0), put<uint64_t>(b, 0), put<uint64_t>(b, 0);
    query_head(b, 78);  // a NewOrder at warehouse 3 (node 0), every item supplied by it
    for (uint64_t v : {2, 3, 2, 9, 0, 0, 0}) put<uint64_t>(b, v);
    for (int i = 0; i < 16; i++) put<uint8_t>(b, 0);
    put<uint64_t>(b, 0), put<uint8_t>(b, 0), put<uint64_t>(b, 62);
    for (uint64_t i = 0; i < 62; i++) put<uint64_t>(b, 1 + i), put<uint64_t>(b, 3), put<uint64_t>(b, 5);
    put<uint8_t>(b, 1), put<uint8_t>(b, 0), put<uint64_t>(b, 62), put<uint64_t>(b, 2013);
    return b;
}

int main() {
    int bad = 0;
    dv_tpcc_params tp{};
    tp.num_wh = 4, tp.dist_per_wh = 10, tp.cust_per_dist = 3000, tp.max_items = 100000, tp.max_items_per_txn = 15;
    tp.part_cnt = 2, tp.part_per_txn = 2, tp.wh_update = 1, tp.perc_payment = 0.5, tp.mpr = 1.0;
    dv_wire_cfg cfg{};
    cfg.workload = DV_TPCC, cfg.calvin = 1, cfg.node_id = 1, cfg.node_cnt = 2, cfg.part_cnt = 2, cfg.tpcc = &tp;
    const std::vector<uint8_t> cm = client_mbuf();
    if (cm.size() != 12 + 215 + 215 + 24 * 62) bad |= std::printf("the mbuf is %zu bytes\n", cm.size());
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
        if (whole ? (rc != DV_OK || r.n_txn != 2 || r.n_taken != 1 || r.n_msgs != 3 || wak[0] != 2 || wak[1] != 1)
                  : (rc != DV_ERR_ARG || r.n_taken != 0 || r.n_txn != 0))
            bad |= std::printf("client prefix %zu: rc %d, %u txns\n", len, rc, r.n_txn);
        std::free(p);
    }
    if (!bad) std::printf("ok %zu\n", cm.size() + 1);
    return bad ? 1 : 0;
}
