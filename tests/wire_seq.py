"""Test infrastructure: the CALVIN sequencer as plain Python over wire_fmt.py,
independent of the product's two implementations (csrc/wire.cpp,
csrc/dvcc_wire.hip), to check them.

It restates the rules of dv_wire_sequence / dv_wire_sequence_acks
(include/dvcc.h) from the reference's text: Sequencer::process_txn and
send_next_batch (system/sequencer.cpp:184-326) stamp the k-th CL_QRY of a batch
with txn_id = node_id + node_cnt * k and the batch id, send it to every node
of YCSBQuery::participants (ycsb_query.cpp:157-165) and close the batch with an
RDONE to every node; MessageThread::run (msg_thread.cpp:94-106) packs a
destination's messages greedily into mbufs of 4,096 bytes;
Sequencer::process_ack (sequencer.cpp:55-181) counts CALVIN_ACKs per txn and
answers the client with a CL_RSP when the last arrives.

Messages here are parsed by struct offsets of a CALVIN build (84-byte header),
never by the product's decoder.
"""
import struct

import wire_fmt as W

OK, MORE, ERR = 0, 1, -1
HDR = 84            # rtype, txn_id, batch_id, mq_time, 7 latencies
ACK, RSP = 88, 92   # AckMessage (header + rc), ClientResponseMessage (header + client_startts)
NO_BATCH = 0xFFFFFFFF


def client_query(reqs, parts, client_startts=0, mq_time=0, lat=(0.0,) * 7):
    """A client's CL_QRY in a CALVIN build: txn_id and batch_id UINT64_MAX
    (message.cpp:177-178); mq_time / lat let a test send clocks that the
    sequencer must zero."""
    m = W.ycsb_query(reqs, parts, client_startts, W.U64_MAX, W.U64_MAX)
    return m[:20] + struct.pack("<Q", mq_time) + struct.pack("<7d", *lat) + m[HDR:]


def parse_client_mbuf(b, node_id, node_cnt, n_dest, part_cnt, table, max_req):
    """[(message bytes, src, client_startts, keys)] or None where the mbuf is malformed"""
    if len(b) < 12 or len(b) > W.MSG_MAX:
        return None
    dest, src, cnt = struct.unpack_from("<III", b, 0)
    if dest != node_id or not node_cnt <= src < n_dest or cnt < 1:
        return None
    lim = min(max_req or 128, 128)
    at, out = 12, []
    for _ in range(cnt):
        if at + HDR + 16 > len(b):
            return None
        (rtype,) = struct.unpack_from("<I", b, at)
        cst, np_ = struct.unpack_from("<QQ", b, at + HDR)
        if rtype != W.CL_QRY or np_ > 64:  # (DV_TPCC_MAX_PARTS: the decoder's bound on a partition list)
            return None
        p = at + HDR + 16
        if p + 8 * np_ + 8 > len(b):
            return None
        if any(x >= part_cnt for x in struct.unpack_from(f"<{np_}Q", b, p)):
            return None
        p += 8 * np_
        (n,) = struct.unpack_from("<Q", b, p)
        p += 8
        if n < 1 or n > lim or p + 24 * n > len(b):
            return None
        keys = []
        for i in range(n):
            acc, key = struct.unpack_from("<I4xQ", b, p + 24 * i)
            if acc > 1 or key >= table:
                return None
            keys.append(key)
        p += 24 * n
        out.append((b[at:p], src, cst, keys))
        at = p
    return out if at == len(b) else None


def sequence(mbufs, batch_id, *, node_id, node_cnt, part_cnt, table, n_dest, max_txn, max_req=0, first=0):
    """-> dict(status, n_taken, n_txn, n_msgs, per_dest=[[mbuf bytes]], wait=[(client, startts, acks)])"""
    txns, status, b = [], OK, first
    while b < len(mbufs):
        t = parse_client_mbuf(mbufs[b], node_id, node_cnt, n_dest, part_cnt, table, max_req)
        if t is None:
            status = ERR
            break
        if len(txns) + len(t) > max_txn:
            status = ERR if b == first else MORE
            break
        txns += t
        b += 1
    per_dest = [[] for _ in range(node_cnt)]
    wait, n_msgs = [], 0
    for k, (m, src, cst, keys) in enumerate(txns):
        parts = {(key % part_cnt) % node_cnt for key in keys}
        stamped = W.header(W.CL_QRY, node_id + node_cnt * k, batch_id) + m[HDR:]
        for d in sorted(parts):
            per_dest[d].append(stamped)
        wait.append((src, cst, len(parts)))
        n_msgs += len(parts)
    per_dest = [W.batches(d, node_id, msgs + [W.rdone(batch_id)]) for d, msgs in enumerate(per_dest)]
    return dict(status=status, n_taken=b, n_txn=len(txns), n_msgs=n_msgs, per_dest=per_dest, wait=wait)


def ack_mbuf(dest, src, acks, rc=0):
    """acks: [(txn_id, batch_id)] -> one mbuf of CALVIN_ACKs"""
    return struct.pack("<III", dest, src, len(acks)) + b"".join(
        W.header(W.CALVIN_ACK, t, e) + struct.pack("<I", rc) for t, e in acks)


def ack_mbufs(dest, src, acks, per=46):
    return [ack_mbuf(dest, src, acks[i:i + per]) for i in range(0, len(acks), per)]


def parse_ack_mbuf(b, node_id, node_cnt):
    """[(txn_id, batch_id)] or None where the mbuf's form is wrong"""
    if len(b) < 12 or len(b) > W.MSG_MAX:
        return None
    dest, src, cnt = struct.unpack_from("<III", b, 0)
    if dest != node_id or src >= node_cnt or not 1 <= cnt <= 46 or len(b) != 12 + ACK * cnt:
        return None
    out = []
    for i in range(cnt):
        rtype, txn_id, bid = struct.unpack_from("<IQQ", b, 12 + ACK * i)
        if rtype != W.CALVIN_ACK or bid == W.U64_MAX:
            return None
        out.append((txn_id, bid))
    return out


def acks(mbufs, batch_id, wait, *, node_id, node_cnt, n_dest):
    """wait: [(client, startts, acks)] -> dict(status, first_bad, n_acks,
    n_skipped, wait (the new list), done (txns in answering order), replies
    (mbuf bytes)); a refused call leaves wait as it was."""
    refused = dict(status=ERR, first_bad=NO_BATCH, n_acks=0, n_skipped=0, wait=list(wait), done=[], replies=[])
    cnt, last, n_acks, n_skipped, pos = {}, {}, 0, 0, 0
    for b, mb in enumerate(mbufs):
        a = parse_ack_mbuf(mb, node_id, node_cnt)
        if a is not None:
            for txn_id, bid in a:
                if bid != batch_id:
                    n_skipped += 1
                elif txn_id % node_cnt != node_id or txn_id // node_cnt >= len(wait):
                    a = None
                    break
                else:
                    k = txn_id // node_cnt
                    cnt[k] = cnt.get(k, 0) + 1
                    last[k] = pos
                    n_acks += 1
                pos += 1
        if a is None:
            return dict(refused, first_bad=b)
    if any(c > wait[k][2] for k, c in cnt.items()):
        return refused
    done = sorted((k for k, c in cnt.items() if c == wait[k][2]), key=lambda k: last[k])
    if any(wait[k][0] >= n_dest for k in done):
        return refused
    new = [(c, s, a - cnt.get(k, 0)) for k, (c, s, a) in enumerate(wait)]
    replies = []
    for d in sorted({wait[k][0] for k in done}):
        msgs = [W.header(W.CL_RSP, node_id + node_cnt * k, W.U64_MAX) + struct.pack("<Q", wait[k][1])
                for k in done if wait[k][0] == d]
        replies += W.batches(d, node_id, msgs)
    return dict(status=OK, first_bad=NO_BATCH, n_acks=n_acks, n_skipped=n_skipped, wait=new, done=done,
                replies=replies)


def parse_rsp_mbuf(b):
    """(dest, src, [(txn_id, batch_id, client_startts)]) of a mbuf of 92-byte CL_RSPs; everything else must be 0"""
    dest, src, cnt = struct.unpack_from("<III", b, 0)
    assert len(b) == 12 + RSP * cnt, (len(b), cnt)
    out = []
    for i in range(cnt):
        at = 12 + RSP * i
        rtype, txn_id, bid = struct.unpack_from("<IQQ", b, at)
        assert rtype == W.CL_RSP and b[at + 20:at + HDR] == bytes(64)
        out.append((txn_id, bid, struct.unpack_from("<Q", b, at + HDR)[0]))
    return dest, src, out


def queue(mbufs):
    """mbufs (bytes) back to back as a receive queue holds them: (uint8 array, u64 offsets)"""
    import numpy as np
    off = np.zeros(len(mbufs) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in mbufs]) if mbufs else []
    return np.frombuffer(b"".join(mbufs) or b"\0", np.uint8)[:int(off[-1])].copy(), off


# ---- cases shared by the CPU tests (host functions against this model) and
# the GPU tests (device entries against the host functions)
def txn(keys, part_cnt, cst=0, wr=1, **kw):
    """a client's CL_QRY over keys, partitions as YCSBQuery's ascending set"""
    return client_query([(wr if i & 1 else 0, k) for i, k in enumerate(keys)], sorted({k % part_cnt for k in keys}),
                        cst, **kw)


def kw(node_id=0, node_cnt=1, part_cnt=1, table=1 << 20, n_dest=None, max_txn=4096, max_req=0):
    return dict(node_id=node_id, node_cnt=node_cnt, part_cnt=part_cnt, table=table,
                n_dest=node_cnt + 2 if n_dest is None else n_dest, max_txn=max_txn, max_req=max_req)


def clients(msgs, node_id, first_client, n_clients=2, per=None):
    """msgs dealt to n_clients clients in runs of `per` (None: greedy mbufs of one client after the other)"""
    out = []
    if per is None:
        share = (len(msgs) + n_clients - 1) // n_clients if msgs else 0
        for c in range(n_clients):
            out += W.batches(node_id, first_client + c, msgs[c * share:(c + 1) * share])
        return out
    for i in range(0, len(msgs), per):
        out += W.batches(node_id, first_client + (i // per) % n_clients, msgs[i:i + per])
    return out


def random_txns(rng, n, part_cnt, table, sizes=(1, 2, 3, 10, 16, 40), clocks=True):
    out = []
    for t in range(n):
        r = int(rng.choice(sizes))
        keys = [int(x) for x in rng.integers(0, table, r)]
        extra = dict(mq_time=int(rng.integers(1, 1 << 40)), lat=tuple(rng.random(7))) if clocks else {}
        out.append(txn(keys, part_cnt, cst=1000 + t, **extra))
    return out


def sized_queue(n_msgs, size):
    """n_msgs CL_QRYs of `size` bytes to one node from two clients (part_cnt 2):
    260 bytes are 15 to an mbuf, 244 are 16"""
    np_, reqs = {260: (1, 6), 244: (2, 5)}[size]
    msgs = [client_query([(i & 1, 2 * i + (j & (np_ - 1))) for j in range(reqs)], list(range(np_)), i)
            for i in range(n_msgs)]
    assert all(len(m) == size for m in msgs)
    return clients(msgs, 0, 1, 2)


def sequence_cases():
    """[(name, mbufs, batch_id, kw)]: well-formed queues at the edges the rules have"""
    import numpy as np
    rng = np.random.default_rng(7)
    cs = []
    for n in (0, 1, 2):
        k = kw(node_id=1, node_cnt=2, part_cnt=2)
        cs.append((f"txns{n}", clients([txn([5 + i, 8], 2, cst=i) for i in range(n)], 1, 2), 3, k))
    cs.append(("one_node", clients(random_txns(rng, 50, 1, 1 << 20), 0, 1), 9, kw()))
    cs.append(("two_nodes", clients(random_txns(rng, 60, 2, 1 << 20), 0, 2), 10, kw(node_cnt=2, part_cnt=2)))
    # 64 nodes, a 64-request txn naming every one; part_cnt 128 folds two partitions on a node
    k = kw(node_id=63, node_cnt=64, part_cnt=128, n_dest=70)
    msgs = [txn(list(range(64)), 128, cst=1), txn([64 + 3, 5], 128, cst=2), txn(list(range(100, 228, 2)), 128, cst=3)]
    cs.append(("nodes64", clients(msgs + random_txns(rng, 30, 128, 1 << 20), 63, 64, 3), 11, k))
    # a destination without a txn: the RDONE alone
    cs.append(("idle_dest", clients([txn([0, 3, 6], 3, cst=i) for i in range(5)], 0, 3), 12,
               kw(node_cnt=3, part_cnt=3)))
    # 2,516 + 1,484 + the 84-byte RDONE + the 12-byte header = 4,096: the RDONE fills the mbuf
    fill = [txn(list(range(100)), 1, cst=1), txn(list(range(57)), 1, cst=2)]
    assert [len(m) for m in fill] == [2516, 1484]
    cs.append(("rdone_fills", clients(fill, 0, 1, 1, per=1), 13, kw()))
    # 8 bytes more (a second partition): the RDONE opens an mbuf of its own
    cs.append(("rdone_alone", clients([txn(list(range(100)), 2, cst=1), txn(list(range(0, 114, 2)), 2, cst=2)],
                                      0, 1, 1, per=1), 14, kw(part_cnt=2)))
    small = [txn([i], 1, cst=i) for i in range(29)]  # 29 x 140 = 4,060; + 84 > 4,084
    assert all(len(m) == 140 for m in small)
    cs.append(("rdone_alone_29", clients(small, 0, 1, 2), 15, kw()))
    # sizes mixed so that every destination cuts elsewhere
    cs.append(("mixed_cuts", clients(random_txns(rng, 400, 12, 1 << 20, sizes=(1, 4, 9, 33, 80, 128)), 2, 5, 3, per=7),
               16, kw(node_id=2, node_cnt=5, part_cnt=12, n_dest=9)))
    return cs


def malformed_cases():
    """[(name, mbufs, kw, n_taken)]: one malformed mbuf among good ones"""
    k = kw(node_id=0, node_cnt=2, part_cnt=2, table=1000, max_req=10)
    good = lambda src=2, n=3: W.batches(0, src, [txn([1 + i, 4], 2, cst=i) for i in range(n)])[0]  # noqa: E731
    mb = lambda src, msgs, dest=0, cnt=None: (  # noqa: E731
        struct.pack("<III", dest, src, len(msgs) if cnt is None else cnt) + b"".join(msgs))
    q = txn([1, 2], 2)
    bad = {
        "src_server": mb(1, [q]), "src_at_n_dest": mb(4, [q]), "dest_other": mb(2, [q], dest=1),
        "count_zero": mb(2, [], cnt=0), "count_more": mb(2, [q], cnt=2), "count_less": mb(2, [q, q], cnt=1),
        "rdone_inside": mb(2, [q, W.rdone(5)]), "rdone_alone": mb(2, [W.rdone(5)]),
        "no_request": mb(2, [client_query([], [0])]), "truncated": mb(2, [q])[:-1], "trailing": mb(2, [q]) + b"\0",
        "rtype": mb(2, [struct.pack("<I", W.CL_RSP) + q[4:]]), "key_range": mb(2, [txn([1000], 2)]),
        "acctype": mb(2, [client_query([(2, 1)], [1])]), "partition": mb(2, [client_query([(0, 1)], [2])]),
        "too_long": mb(2, [txn(list(range(11)), 2)]),
        "req_count_huge": mb(2, [q[:HDR + 16 + 16] + struct.pack("<Q", (1 << 61) + 2) + q[HDR + 40:]]),
        "part_count_huge": mb(2, [q[:HDR + 8] + struct.pack("<Q", (1 << 61) + 2) + q[HDR + 16:]]),
        "short": b"\0" * 11,
    }
    out = []
    for name, b in bad.items():
        out.append((name + "_first", [b, good()], k, 0))
        out.append((name + "_last", [good(), good(3, 2), b], k, 2))
    out.append(("middle", [good(), bad["src_server"], good()], k, 1))
    return out


def ack_cases():
    """[(name, wait, batch_id, calls, kw)]: wait = [(client, startts, acks)], calls = [[mbuf]] applied in turn"""
    E, nid, nc = 21, 1, 3
    k = dict(node_id=nid, node_cnt=nc, n_dest=6)
    tid = lambda t: nid + nc * t  # noqa: E731
    wait = [(3 + t % 3, 100 + t, 1 + t % 3) for t in range(200)]
    per_node = [[(tid(t), E) for t in range(200) if wait[t][2] > s] for s in range(nc)]
    cs = [("all_in_one", wait, E, [sum((ack_mbufs(nid, s, per_node[s]) for s in range(nc)), [])], k),
          ("node_per_call", wait, E, [ack_mbufs(nid, s, per_node[s]) for s in range(nc)], k),
          ("reversed_nodes", wait, E, [sum((ack_mbufs(nid, s, per_node[s][::-1]) for s in (2, 1, 0)), [])], k)]
    mixed = [(tid(t), E if i % 3 else E + 1 + i % 2) for i, t in enumerate(list(range(200)) * 2)]
    cs.append(("other_batches", wait, E, [ack_mbufs(nid, 0, mixed, per=45)], k))
    cs.append(("mbuf_45_46", [(4, 7, 1)] * 91, E, [[ack_mbuf(nid, 0, [(tid(t), E) for t in range(45)]),
                                                     ack_mbuf(nid, 2, [(tid(t), E) for t in range(45, 91)])]], k))
    cs.append(("empty_call", wait[:5], E, [[]], k))
    # refused calls: nothing changes
    one = [(3, 9, 1), (4, 8, 2)]
    cs.append(("over_ack", one, E, [[ack_mbuf(nid, 0, [(tid(0), E), (tid(1), E)]), ack_mbuf(nid, 1, [(tid(0), E)])]], k))
    cs.append(("foreign_txn", one, E, [[ack_mbuf(nid, 0, [(tid(1), E)]), ack_mbuf(nid, 0, [(tid(0) + 1, E)])]], k))
    cs.append(("txn_at_n_txn", one, E, [[ack_mbuf(nid, 0, [(tid(2), E)])]], k))
    cs.append(("mbuf_47", [(4, 7, 1)] * 47, E, [[ack_mbuf(nid, 0, [(tid(t), E) for t in range(47)])]], k))
    cs.append(("src_client", one, E, [[ack_mbuf(nid, 3, [(tid(0), E)])]], k))
    cs.append(("dest_other", one, E, [[ack_mbuf(0, 0, [(tid(0), E)])]], k))
    cs.append(("no_batch_id", one, E, [[ack_mbuf(nid, 0, [(tid(0), W.U64_MAX)])]], k))
    cs.append(("not_an_ack", one, E, [[ack_mbuf(nid, 0, [(tid(0), E)])[:12] + struct.pack("<I", W.CL_RSP)
                                        + ack_mbuf(nid, 0, [(tid(0), E)])[16:]]], k))
    cs.append(("length", one, E, [[ack_mbuf(nid, 0, [(tid(0), E)]) + b"\0\0\0\0"]], k))
    cs.append(("client_at_n_dest", [(6, 1, 1)], E, [[ack_mbuf(nid, 0, [(tid(0), E)])]], k))
    return cs
