// The workspace layouts of the wire ingests (csrc/dvcc_wire_layout.h) on the
// host: for every nb named on the command line and both workspaces, every
// field aligned to its element type, no two fields overlapping, the last one
// ending at or below the byte count the same routine reports without a base,
// and nb = 0 laid out as nb = 1.  The sizes below are what the kernels index:
// stated here on their own, not taken from the header's routine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dvcc_wire_layout.h"

using namespace dvcc;

struct Field {
    const char *name;
    const void *p;
    uint64_t bytes, align;
};

template <class T>
static Field field(const char *name, const T *p, uint64_t n) {
    return Field{name, p, n * sizeof(T), alignof(T)};
}

static std::vector<Field> fields(const WireWs &w, uint64_t n, uint64_t nc, uint64_t stride) {
    return {{"res", w.res, kWireResBytes, 8}, field("first", w.first, 2),  field("moff", w.moff, n * stride),
            field("bt", w.bt, n),            field("ba", w.ba, n),        field("bm", w.bm, n),
            field("ct", w.ct, nc),           field("ca", w.ca, nc),       field("cm", w.cm, nc)};
}

static int check(const char *what, uint32_t nb, const std::vector<Field> &fs, const char *base, uint64_t bytes) {
    int bad = 0;
    for (const Field &f : fs) {
        const char *p = static_cast<const char *>(f.p);
        if (p < base || reinterpret_cast<uintptr_t>(p) % f.align || p + f.bytes > base + bytes) {
            std::printf("%s nb=%u: %s misaligned or outside its %llu bytes\n", what, nb, f.name, (unsigned long long)bytes);
            bad = 1;
        }
        for (const Field &g : fs) {
            const char *q = static_cast<const char *>(g.p);
            if (&f != &g && p < q + g.bytes && q < p + f.bytes) {
                std::printf("%s nb=%u: %s overlaps %s\n", what, nb, f.name, g.name);
                bad = 1;
            }
        }
    }
    return bad;
}

template <class Ws, class Layout>
static int same_as_one(const char *what, Layout layout) {
    std::vector<uint64_t> mem(1 << 13);
    Ws w0, w1;  // (pointers alone: no padding to compare)
    const uint64_t s0 = layout(mem.data(), 0, w0), s1 = layout(mem.data(), 1, w1);
    if (s0 == s1 && !std::memcmp(&w0, &w1, sizeof(Ws))) return 0;
    return std::printf("%s: nb=0 is not laid out as nb=1\n", what), 1;
}

int main(int argc, char **argv) {
    int bad = same_as_one<WireWs>("client", wire_ws_layout) | same_as_one<WireCalvinWs>("calvin", wire_calvin_ws_layout);
    for (int i = 1; i < argc; i++) {
        const uint32_t nb = (uint32_t)std::strtoul(argv[i], nullptr, 10);
        const uint64_t n = nb ? nb : 1, nc = (n + kWireChunk - 1) / kWireChunk;
        {
            WireWs w;
            const uint64_t bytes = wire_ws_layout(nullptr, nb, w);
            std::vector<uint64_t> mem(bytes / 8 + 1);  // (8-byte aligned, as any device allocation is)
            char *base = reinterpret_cast<char *>(mem.data());
            if (wire_ws_layout(base, nb, w) != bytes) bad |= std::printf("client nb=%u: two sizes\n", nb);
            bad |= check("client", nb, fields(w, n, nc, kWireMaxMsg), base, bytes);
        }
        {
            WireCalvinWs w;
            const uint64_t bytes = wire_calvin_ws_layout(nullptr, nb, w);
            std::vector<uint64_t> mem(bytes / 8 + 1);
            char *base = reinterpret_cast<char *>(mem.data());
            if (wire_calvin_ws_layout(base, nb, w) != bytes) bad |= std::printf("calvin nb=%u: two sizes\n", nb);
            std::vector<Field> fs = fields(w, n, nc, kWireCalvinMaxMsg);
            fs.push_back(field("bid", w.bid, n));
            fs.push_back(field("br", w.br, n));
            fs.push_back(field("cr", w.cr, nc));
            fs.push_back(field("brun", w.brun, n));
            fs.push_back(field("bflag", w.bflag, n));
            bad |= check("calvin", nb, fs, base, bytes);
            if (static_cast<const void *>(w.cres) != w.res) bad |= std::printf("calvin nb=%u: cres is not res\n", nb);
        }
    }
    if (!bad) std::printf("ok %d\n", argc - 1);
    return bad ? 1 : 0;
}
