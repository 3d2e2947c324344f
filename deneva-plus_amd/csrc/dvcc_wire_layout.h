// dvcc_wire_layout.h -- the per-call device words of the wire ingests
// (dvcc_wire.hip) and where each lies in the context's one allocation.  One
// routine walks the field list and either sums the sizes (no base) or assigns
// the pointers, so the allocation's size and the carve cannot disagree.  Host-compilable: <cstdint>, dvcc.h and the constants below.
#pragma once
#include <cstdint>

#include "dvcc.h"

namespace dvcc {

// k_wire_check takes kWireWave batches per workgroup (a wave each), the scan
// kWireChunk batches per chunk, the reply compaction kReplyTile txns per tile.
constexpr uint32_t kWireWave = 4;
constexpr uint32_t kWireChunk = 256 * 12;  // (block_chunk_scan256's register path)
constexpr uint32_t kWireMaxMsg = 40;       // messages of a 4,096-byte batch (100 bytes each at least)
// CALVIN: the header carries batch_id (84 bytes), an RDONE is the header alone,
// so an mbuf holds up to kWireCalvinMaxMsg messages -- the path's own stride
constexpr uint32_t kWireCalvinMaxMsg = 48;
constexpr uint32_t kReplyTile = 256;
constexpr uint32_t kWireResBytes = 64;  // the plan's record: the context's pinned words

// the per-call words of nb batches (device): carved from one allocation
struct WireWs {
    uint32_t *bt, *ba;       // [nb] txns / accesses per batch, then their prefix inside the chunk
    uint8_t *bm;             // [nb] the batch's longest txn
    uint16_t *moff;          // [nb * stride] message offsets inside the batch
    uint32_t *ct, *ca, *cm;  // [chunks] per chunk: txns, accesses (then their prefixes), longest txn
    uint32_t *first;         // two words: the first malformed batch; CALVIN: the first where the batch ends
    dv_wire_dev_result *res; // kWireResBytes
};
// what the CALVIN plan leaves for the host (pos, status) and for the emit
struct WireCalvinRes {
    dv_wire_calvin_pos pos;
    int32_t status;
    uint32_t n_emit;    // mbufs of the window the emit decodes
    uint32_t last_end;  // the last of them: its messages below this one (its count: all)
    uint32_t pad_;
};
static_assert(sizeof(WireCalvinRes) <= kWireResBytes && sizeof(dv_wire_dev_result) <= kWireResBytes,
              "the context's pinned words");
// CALVIN: a batch is an mbuf, its counts those of its run
struct WireCalvinWs : WireWs {
    uint32_t *br;    // [nb] RDONEs of the mbuf's run, then their prefix inside the chunk
    uint64_t *bid;   // [nb] the batch id of the mbuf's first message from the cursor
    uint8_t *brun;   // [nb] the run's length in messages
    uint8_t *bflag;  // [nb] the message behind the run: 0 none, 1 a later batch, 2 an earlier one
    uint32_t *cr;    // [chunks] RDONEs per chunk, then their prefix
    WireCalvinRes *cres;  // (res, as the record it holds here)
};

// The sequencer (dv_wire_sequence_device): a batch is a client mbuf of at most
// kWireMaxMsg CL_QRYs (108 bytes each at least), bm its message count, ba the
// messages it sends (its txns' participants).  A destination's messages and
// its RDONE are a list; the lists lie back to back, destination d's at lb[d] =
// sum over d' < d of (dtot[d'] + 2).  The cut search takes kSeqTile list
// entries per workgroup; a message that no longer fits an mbuf lies fewer than
// kSeqReach entries behind the mbuf's first.
constexpr uint32_t kSeqTile = 256;
constexpr uint32_t kSeqReach = 64;
constexpr uint32_t kSeqMaxTxn = 1u << 20;  // (a destination's bytes stay in 32 bits)
constexpr uint32_t kSeqMbufParts = (DV_WIRE_MSG_MAX - DV_WIRE_HDR) / 24;  // requests, so participants, of an mbuf
static_assert((uint64_t)kSeqMaxTxn * (DV_WIRE_MSG_MAX - DV_WIRE_HDR) + 84 + DV_WIRE_MSG_MAX < (1ull << 32),
              "a destination's bytes and a cut's target in 32 bits");
struct WireSeqPlan {  // what the first plan leaves for the kernels behind it
    uint32_t taken, n_txn, n_msgs;
    int32_t status;
    uint32_t refused, pad_[3];  // the second plan: the outputs do not fit, nothing is written
};
struct WireSeqWs : WireWs {
    WireSeqPlan *plan;
    dv_wire_seq_result *sres;  // (res, as the record it holds here)
    uint64_t *mmask;           // [nb * kWireMaxMsg] a message's participants
    uint16_t *msz;             // [nb * kWireMaxMsg] its bytes
    uint32_t *dcnt, *dbyt;     // [nodes * nb] a destination's messages / bytes in mbuf b, then those in front of it
    uint32_t *dtot, *dtotb;    // [nodes] a destination's messages / their bytes
    uint32_t *dmb, *dMB;       // [nodes] its mbufs / the mbufs in front of its first
    uint64_t *dDB;             // [nodes] the bytes in front of its first mbuf
    uint32_t *lS;              // [n_list] a list entry's bytes in front of it in its destination
    uint32_t *ljmp;            // [n_list] from this entry: mbufs opened inside its tile << 8 | where the walk leaves it
    uint64_t *lpos;            // [n_list] the entry's byte in out
    uint32_t *tent, *tmb;      // [nodes * n_tile] where the walk enters a tile, the destination's mbufs in front of it
};
static_assert(sizeof(dv_wire_seq_result) <= kWireResBytes, "the context's pinned words");

// the list entries and tiles per destination that nb mbufs of at most max_txn txns can need
inline uint64_t wire_seq_list_cap(uint32_t nb, uint32_t nodes, uint32_t max_txn) {
    const uint64_t per_mbuf = kSeqMbufParts < (uint64_t)kWireMaxMsg * nodes ? kSeqMbufParts : (uint64_t)kWireMaxMsg * nodes;
    const uint64_t per_txn = nodes < 128 ? nodes : 128;
    const uint64_t a = nb * per_mbuf, b = max_txn * per_txn;
    return (a < b ? a : b) + 2ull * nodes;
}
inline uint32_t wire_seq_tiles(uint32_t nb, uint32_t max_txn) {
    const uint64_t a = (uint64_t)nb * kWireMaxMsg, t = a < max_txn ? a : max_txn;
    return (uint32_t)((t + 1 + kSeqTile - 1) / kSeqTile);
}

// field f: n elements at the cursor, which moves on to the next multiple of 8 bytes
template <class T>
inline void wire_ws_field(char *base, uint64_t &at, T *&f, uint64_t n) {
    f = base ? reinterpret_cast<T *>(base + at) : nullptr;
    at += (n * sizeof(T) + 7) & ~7ull;
}

// The one description of both workspaces: w's fields -- and, for CALVIN, c's
// own (c is w) -- for nb batches (0 as 1) of `stride` messages.  Returns the
// bytes they take; with a base it also points every field into it.
inline uint64_t wire_ws_walk(void *base_, uint32_t nb, uint32_t stride, WireWs &w, WireCalvinWs *c,
                             WireSeqWs *q = nullptr, uint32_t nodes = 0, uint32_t max_txn = 0) {
    const uint64_t n = nb ? nb : 1, nc = (n + kWireChunk - 1) / kWireChunk;
    char *base = static_cast<char *>(base_);
    uint64_t at = 0;
    uint8_t *res;
    wire_ws_field(base, at, res, kWireResBytes);
    w.res = reinterpret_cast<dv_wire_dev_result *>(res);
    wire_ws_field(base, at, w.first, 2);
    if (c) c->cres = reinterpret_cast<WireCalvinRes *>(res);
    if (c) wire_ws_field(base, at, c->bid, n);
    wire_ws_field(base, at, w.moff, n * stride);
    wire_ws_field(base, at, w.bt, n);
    wire_ws_field(base, at, w.ba, n);
    if (c) wire_ws_field(base, at, c->br, n);
    wire_ws_field(base, at, w.ct, nc);
    wire_ws_field(base, at, w.ca, nc);
    if (c) wire_ws_field(base, at, c->cr, nc);
    wire_ws_field(base, at, w.cm, nc);
    wire_ws_field(base, at, w.bm, n);
    if (c) wire_ws_field(base, at, c->brun, n);
    if (c) wire_ws_field(base, at, c->bflag, n);
    if (!q) return at;
    // the sequencer's own (q is w): nodes destinations, lists of wire_seq_list_cap entries
    const uint64_t nl = wire_seq_list_cap((uint32_t)n, nodes, max_txn), ntile = wire_seq_tiles((uint32_t)n, max_txn);
    q->sres = reinterpret_cast<dv_wire_seq_result *>(res);
    uint8_t *plan;
    wire_ws_field(base, at, plan, sizeof(WireSeqPlan));
    q->plan = reinterpret_cast<WireSeqPlan *>(plan);
    wire_ws_field(base, at, q->mmask, n * stride);
    wire_ws_field(base, at, q->msz, n * stride);
    wire_ws_field(base, at, q->dcnt, n * nodes);
    wire_ws_field(base, at, q->dbyt, n * nodes);
    wire_ws_field(base, at, q->dtot, nodes);
    wire_ws_field(base, at, q->dtotb, nodes);
    wire_ws_field(base, at, q->dmb, nodes);
    wire_ws_field(base, at, q->dMB, nodes);
    wire_ws_field(base, at, q->dDB, nodes);
    wire_ws_field(base, at, q->lS, nl);
    wire_ws_field(base, at, q->ljmp, nl);
    wire_ws_field(base, at, q->lpos, nl);
    wire_ws_field(base, at, q->tent, ntile * nodes);
    wire_ws_field(base, at, q->tmb, ntile * nodes);
    return at;
}

// The reply packer's words (dv_wire_respond_device) for nt tiles of kReplyTile
// txns over n_dest destinations: the stable multi-split's counts, destination-
// major so that one destination's tiles are contiguous for its scan.
struct ReplyWs {
    dv_wire_rsp_result *res;  // kWireResBytes
    uint32_t *err;            // one word: an answered txn's node or a list's index out of range
    uint32_t *tot;            // [n_dest] replies per destination
    uint32_t *dmb, *dmsg;     // [n_dest] mbufs / messages in front of the destination's first
    uint32_t *cnt;            // [n_dest * nt] per tile, then the destination's replies in front of the tile
};
static_assert(sizeof(dv_wire_rsp_result) <= kWireResBytes, "the context's pinned words");

inline uint64_t reply_ws_layout(void *base_, uint32_t nt, uint32_t n_dest, ReplyWs &w) {
    char *base = static_cast<char *>(base_);
    uint64_t at = 0;
    uint8_t *res;
    wire_ws_field(base, at, res, kWireResBytes);
    w.res = reinterpret_cast<dv_wire_rsp_result *>(res);
    wire_ws_field(base, at, w.err, 1);
    wire_ws_field(base, at, w.tot, n_dest);
    wire_ws_field(base, at, w.dmb, n_dest);
    wire_ws_field(base, at, w.dmsg, n_dest);
    wire_ws_field(base, at, w.cnt, (uint64_t)n_dest * (nt ? nt : 1));
    return at;
}

// The sequencer's acks (dv_wire_sequence_acks_device): the reply packer's words
// for the txns that can complete, then its own for nb ack mbufs against n_txn
// wait-list entries.  [zeroed, zeroed + zeroed_bytes) is cleared per call.
struct AckWs {
    ReplyWs r;
    dv_wire_seq_ack_result *ares;  // kWireResBytes
    uint32_t *first;               // the first malformed mbuf
    uint8_t *zeroed;
    uint64_t zeroed_bytes;
    uint32_t *err2;                // a txn over-acked, a completed txn's client out of range
    uint32_t *counts;              // acks of the batch, of other batches, completed txns
    uint32_t *acnt, *alast;        // [n_txn] a txn's acks in the call, the position of its last
    uint32_t *bt;                  // [nb] completing acks of the mbuf, then those in front of it
    uint32_t *done;                // [n_cap] the completed txns in completing order
};
static_assert(sizeof(dv_wire_seq_ack_result) <= kWireResBytes, "the context's pinned words");

// the txns nb mbufs of at most 46 acks can complete
inline uint32_t ack_done_cap(uint32_t nb, uint32_t n_txn) {
    const uint64_t a = (uint64_t)nb * 46;
    return a < n_txn ? (uint32_t)a : n_txn;
}

inline uint64_t ack_ws_layout(void *base_, uint32_t nb, uint32_t n_txn, uint32_t n_dest, AckWs &w) {
    char *base = static_cast<char *>(base_);
    const uint32_t n_cap = ack_done_cap(nb, n_txn);
    uint64_t at = reply_ws_layout(base_, (n_cap + kReplyTile - 1) / kReplyTile, n_dest, w.r);
    uint8_t *res;
    wire_ws_field(base, at, res, kWireResBytes);
    w.ares = reinterpret_cast<dv_wire_seq_ack_result *>(res);
    wire_ws_field(base, at, w.first, 2);
    const uint64_t z0 = at;
    wire_ws_field(base, at, w.zeroed, 0);
    wire_ws_field(base, at, w.err2, 2);
    wire_ws_field(base, at, w.counts, 4);
    wire_ws_field(base, at, w.acnt, n_txn ? n_txn : 1);
    wire_ws_field(base, at, w.alast, n_txn ? n_txn : 1);
    w.zeroed_bytes = at - z0;
    wire_ws_field(base, at, w.bt, nb ? nb : 1);
    wire_ws_field(base, at, w.done, n_cap ? n_cap : 1);
    return at;
}

inline uint64_t wire_ws_layout(void *base, uint32_t nb, WireWs &w) {
    return wire_ws_walk(base, nb, kWireMaxMsg, w, nullptr);
}

inline uint64_t wire_calvin_ws_layout(void *base, uint32_t nb, WireCalvinWs &w) {
    return wire_ws_walk(base, nb, kWireCalvinMaxMsg, w, &w);
}

inline uint64_t wire_seq_ws_layout(void *base, uint32_t nb, uint32_t nodes, uint32_t max_txn, WireSeqWs &w) {
    return wire_ws_walk(base, nb, kWireMaxMsg, w, nullptr, &w, nodes, max_txn);
}

}  // namespace dvcc
