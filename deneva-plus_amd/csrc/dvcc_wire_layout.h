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

// field f: n elements at the cursor, which moves on to the next multiple of 8 bytes
template <class T>
inline void wire_ws_field(char *base, uint64_t &at, T *&f, uint64_t n) {
    f = base ? reinterpret_cast<T *>(base + at) : nullptr;
    at += (n * sizeof(T) + 7) & ~7ull;
}

// The one description of both workspaces: w's fields -- and, for CALVIN, c's
// own (c is w) -- for nb batches (0 as 1) of `stride` messages.  Returns the
// bytes they take; with a base it also points every field into it.
inline uint64_t wire_ws_walk(void *base_, uint32_t nb, uint32_t stride, WireWs &w, WireCalvinWs *c) {
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

inline uint64_t wire_ws_layout(void *base, uint32_t nb, WireWs &w) {
    return wire_ws_walk(base, nb, kWireMaxMsg, w, nullptr);
}

inline uint64_t wire_calvin_ws_layout(void *base, uint32_t nb, WireCalvinWs &w) {
    return wire_ws_walk(base, nb, kWireCalvinMaxMsg, w, &w);
}

}  // namespace dvcc
