"""Test infrastructure: the CALVIN sequencer over TPC-C client mbufs as plain
Python over wire_fmt.tpcc_query, independent of the product's two
implementations (csrc/wire.cpp, csrc/dvcc_wire.hip), to check them -- what
tests/wire_seq.py is for YCSB.

It restates, from the reference's text, what a TPC-C cfg changes in
dv_wire_sequence (include/dvcc.h): the field checks of a
TPCCClientQueryMessage (message.cpp:620-687 and the txn manager's walks of
items[0 .. ol_cnt)), and TPCCQuery::participants (benchmarks/tpcc_query.cpp:
67-90): GET_NODE_ID(wh_to_part(w)) of w_id, a Payment's c_w_id, a NewOrder's
supply warehouses.  Messages are parsed by struct offsets of a CALVIN build
(84-byte header), never by the product's decoder.  A CALVIN-build message is
207 + 8 np + 24 n bytes: always 3 mod 4 and 7 mod 8.
"""
import struct

import wire_fmt as W

OK, MORE, ERR = 0, 1, -1
HDR = 84
BODY, TAIL, ITEM = 89, 18, 24  # up to and with the item count; rbk, remote, ol_cnt, o_entry_d; Item_no
MAX_OL, MAX_PARTS = 62, 64
OPERAND = 1 << 56


def size(np_, n):
    return 207 + 8 * np_ + 24 * n


def tp(num_wh=4, dist=10, cust=3000, items=100000, part_cnt=1):
    """the knobs the checks and the participant rule follow"""
    return dict(num_wh=num_wh, dist=dist, cust=cust, items=items, part_cnt=part_cnt)


def query(q, cst=0, mq_time=0, lat=(0.0,) * 7):
    """a client's CL_QRY in a CALVIN build: txn_id and batch_id UINT64_MAX;
    mq_time / lat let a test send clocks that the sequencer must zero"""
    m = W.tpcc_query(q, cst, W.U64_MAX, W.U64_MAX)
    m = m[:20] + struct.pack("<Q", mq_time) + struct.pack("<7d", *lat) + m[HDR:]
    assert len(m) == size(len(q.get("parts", [])), len(q.get("items", [])))
    return m


def payment(w, c_w=None, cst=0, parts=(0,), items=(), **f):
    q = dict(txn_type=1, w_id=w, d_id=1 + w % 10, c_id=7, d_w_id=w, c_w_id=w if c_w is None else c_w, c_d_id=2,
             h_amount=1234, parts=list(parts), items=list(items))
    clocks = {k: f.pop(k) for k in ("mq_time", "lat") if k in f}
    q.update(f)
    return query(q, cst, **clocks)


def new_order(w, items, cst=0, parts=(0,), **f):
    q = dict(txn_type=2, w_id=w, d_id=1 + w % 10, c_id=9, parts=list(parts), items=list(items), ol_cnt=len(items),
             o_entry_d=2013, rbk=True, remote=True)
    clocks = {k: f.pop(k) for k in ("mq_time", "lat") if k in f}
    q.update(f)
    return query(q, cst, **clocks)


def parse_message(b, at, part_cnt, t):
    """(end, client_startts, warehouses that name a participant) of the CL_QRY at b[at:], None where it is refused"""
    if at + HDR + 16 > len(b):
        return None
    (rtype,) = struct.unpack_from("<I", b, at)
    cst, np_ = struct.unpack_from("<QQ", b, at + HDR)
    if rtype != W.CL_QRY or np_ > MAX_PARTS:
        return None
    p = at + HDR + 16
    if p + 8 * np_ + BODY > len(b):
        return None
    if any(x >= part_cnt for x in struct.unpack_from(f"<{np_}Q", b, p)):
        return None
    p += 8 * np_
    tt, w, d, c, _d_w, c_w, c_d = struct.unpack_from("<7Q", b, p)
    c_last = b[p + 56:p + 72]
    h, by_name, n = struct.unpack_from("<QBQ", b, p + 72)
    if n > MAX_OL or p + BODY + ITEM * n + TAIL > len(b):
        return None
    items = [struct.unpack_from("<3Q", b, p + BODY + ITEM * i) for i in range(n)]
    (ol_cnt,) = struct.unpack_from("<Q", b, p + BODY + ITEM * n + 2)
    end = p + BODY + ITEM * n + TAIL
    wh_ok = lambda x: 1 <= x <= t["num_wh"]  # noqa: E731
    if not wh_ok(w) or not 1 <= d <= t["dist"]:
        return None
    if tt == 1:  # (a Payment's items are skipped unchecked and name no participant)
        if not wh_ok(c_w) or not 1 <= c_d <= t["dist"] or h >= OPERAND:
            return None
        if by_name and 0 not in c_last:
            return None
        if not by_name and not 1 <= c <= t["cust"]:
            return None
        return end, cst, [w, c_w]
    if tt == 2:
        if ol_cnt != n or n < 1 or not 1 <= c <= t["cust"]:
            return None
        if any(not 1 <= i <= t["items"] or not wh_ok(s) or q >= OPERAND for i, s, q in items):
            return None
        return end, cst, [w] + [s for _, s, _ in items]
    return None


def parse_client_mbuf(b, node_id, node_cnt, n_dest, part_cnt, t):
    """[(message bytes, src, client_startts, participants)] or None where the mbuf is malformed"""
    if len(b) < 12 or len(b) > W.MSG_MAX:
        return None
    dest, src, cnt = struct.unpack_from("<III", b, 0)
    if dest != node_id or not node_cnt <= src < n_dest or cnt < 1:
        return None
    at, out = 12, []
    for _ in range(cnt):
        m = parse_message(b, at, part_cnt, t)
        if m is None:
            return None
        end, cst, whs = m
        out.append((b[at:end], src, cst, {((w - 1) % t["part_cnt"]) % node_cnt for w in whs}))
        at = end
    return out if at == len(b) else None


def sequence(mbufs, batch_id, *, node_id, node_cnt, part_cnt, tp, n_dest, max_txn, first=0):
    """-> dict(status, n_taken, n_txn, n_msgs, per_dest=[[mbuf bytes]], wait=[(client, startts, acks)])"""
    txns, status, b = [], OK, first
    while b < len(mbufs):
        t = parse_client_mbuf(mbufs[b], node_id, node_cnt, n_dest, part_cnt, tp)
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
    for k, (m, src, cst, parts) in enumerate(txns):
        stamped = W.header(W.CL_QRY, node_id + node_cnt * k, batch_id) + m[HDR:]
        for d in sorted(parts):
            per_dest[d].append(stamped)
        wait.append((src, cst, len(parts)))
        n_msgs += len(parts)
    per_dest = [W.batches(d, node_id, msgs + [W.rdone(batch_id)]) for d, msgs in enumerate(per_dest)]
    return dict(status=status, n_taken=b, n_txn=len(txns), n_msgs=n_msgs, per_dest=per_dest, wait=wait)


# ---- cases shared by the CPU tests (host function against this model) and
# the GPU tests (device entry against the host function)
def kw(node_id=0, node_cnt=1, part_cnt=1, tp_=None, n_dest=None, max_txn=4096):
    return dict(node_id=node_id, node_cnt=node_cnt, part_cnt=part_cnt, tp=tp_ or tp(),
                n_dest=node_cnt + 2 if n_dest is None else n_dest, max_txn=max_txn)


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


def random_txns(rng, n, part_cnt, t, nps=(0, 1, 2), ns=(1, 5, 15), clocks=True):
    """Payments (a quarter by name, some with leftover items) and NewOrders over every warehouse"""
    out = []
    wh = lambda: int(rng.integers(1, t["num_wh"] + 1))  # noqa: E731
    item = lambda: (int(rng.integers(1, t["items"] + 1)), wh(), int(rng.integers(1, 11)))  # noqa: E731
    for i in range(n):
        parts = [int(x) for x in rng.integers(0, part_cnt, int(rng.choice(nps)))]
        extra = dict(mq_time=int(rng.integers(1, 1 << 40)), lat=tuple(rng.random(7))) if clocks else {}
        if rng.random() < 0.5:
            left = [item() for _ in range(int(rng.choice((0, 0, 3))))]
            name = dict(by_last_name=True, c_last=b"BARBARBAR", c_id=0) if rng.random() < 0.25 else {}
            out.append(payment(wh(), wh(), cst=1000 + i, parts=parts, items=left, ol_cnt=len(left), **name, **extra))
        else:
            out.append(new_order(wh(), [item() for _ in range(int(rng.choice(ns)))], cst=1000 + i, parts=parts,
                                 **extra))
    return out


def sized_queue(n_msgs, sz):
    """n_msgs CL_QRYs of `sz` bytes to one node from two clients: 215 (a
    Payment, np = 1) are 18 to an mbuf, 1,703 (a 62-item NewOrder, np = 1) are 2"""
    if sz == 215:
        msgs = [payment(1 + i % 4, cst=i) for i in range(n_msgs)]
    else:
        msgs = [new_order(1 + i % 4, [(1 + i + j, 1 + j % 4, j) for j in range(62)], cst=i) for i in range(n_msgs)]
    assert all(len(m) == sz for m in msgs)
    return clients(msgs, 0, 1, 2)


def filling(k, a, more=0):
    """k NewOrders whose np + 3 n sum to a (+ more partitions on the last): 207 k + 8 a message bytes"""
    n = min(MAX_OL, max(1, a // k // 3))
    rest = a - 3 * n * k
    assert 0 <= rest <= MAX_PARTS - more
    msgs = [new_order(1, [(1 + j, 1, j) for j in range(n)], cst=i,
                      parts=[0] * ((rest if i == 0 else 0) + (more if i == k - 1 else 0))) for i in range(k)]
    assert sum(len(m) for m in msgs) == 207 * k + 8 * (a + more)
    return msgs


def sequence_cases():
    """[(name, mbufs, batch_id, kw)]: well-formed queues at the edges the rules have"""
    import numpy as np
    rng = np.random.default_rng(11)
    cs = []
    t2 = tp(num_wh=4, part_cnt=2)
    for n in (0, 1, 2):
        k = kw(node_id=1, node_cnt=2, part_cnt=2, tp_=t2)
        cs.append((f"txns{n}", clients([payment(1 + i, 2, cst=i) for i in range(n)], 1, 2), 3, k))
    cs.append(("one_node", clients(random_txns(rng, 50, 1, tp()), 0, 1), 9, kw()))
    cs.append(("two_nodes", clients(random_txns(rng, 60, 2, t2), 0, 2), 10, kw(node_cnt=2, part_cnt=2, tp_=t2)))
    # 64 nodes: a 62-item NewOrder naming 63 of them, np 64; part_cnt 100 folds partitions on a node
    t64 = tp(num_wh=128, part_cnt=100)
    k = kw(node_id=63, node_cnt=64, part_cnt=100, tp_=t64, n_dest=70)
    msgs = [new_order(1, [(1 + j, 2 + j, j) for j in range(62)], cst=1, parts=list(range(64))),
            new_order(65, [(5, 102, 1)], cst=2, parts=[]), payment(128, 100, cst=3, parts=[99])]
    cs.append(("nodes64", clients(msgs + random_txns(rng, 30, 100, t64, nps=(0, 1, 64), ns=(1, 15, 62)), 63, 64, 3), 11, k))
    # a destination without a txn: the RDONE alone
    t3 = tp(num_wh=3, part_cnt=3)
    cs.append(("idle_dest", clients([payment(1, 3, cst=i) for i in range(5)], 0, 3), 12,
               kw(node_cnt=3, part_cnt=3, tp_=t3)))
    # tpcc part_cnt 5 over 3 nodes: above node_cnt and no multiple of it
    t5 = tp(num_wh=11, part_cnt=5)
    cs.append(("parts_fold", clients(random_txns(rng, 80, 5, t5), 1, 3, 3, per=4), 13,
               kw(node_id=1, node_cnt=3, part_cnt=5, tp_=t5, n_dest=7)))
    # np 0 / 1 / 64, n 0 on a Payment / 1 / 15 / 62
    t8 = tp(num_wh=16, part_cnt=8)
    msgs = [payment(3, 12, cst=1, parts=[]), payment(4, 4, cst=2, parts=[7]), payment(5, 9, cst=3, parts=[1] * 64),
            new_order(6, [(9, 15, 2)], cst=4, parts=[]), new_order(7, [(1 + j, 1 + j, j) for j in range(15)], cst=5),
            new_order(8, [(1 + j, 1 + j % 16, j) for j in range(62)], cst=6, parts=list(range(8)) * 8)]
    assert [len(m) for m in msgs] == [size(0, 0), size(1, 0), size(64, 0), size(0, 1), size(1, 15), size(64, 62)]
    cs.append(("mixed_np_n", clients(msgs * 3, 2, 5, 2, per=4), 14, kw(node_id=2, node_cnt=5, part_cnt=8, tp_=t8, n_dest=8)))
    # sizes mixed so that every destination cuts elsewhere
    cs.append(("mixed_cuts", clients(random_txns(rng, 400, 8, t8, nps=(0, 1, 3, 64), ns=(1, 4, 9, 33, 62)), 2, 5, 3, per=7),
               16, kw(node_id=2, node_cnt=5, part_cnt=8, tp_=t8, n_dest=9)))
    return cs


def fill_cases():
    """[(name, mbufs, batch_id, kw, mbufs out, the last mbuf's bytes)]: a
    destination's mbuf filled to exactly 4,096 bytes by its messages alone
    (4 or 12 of them: 207 k + 8 a = 4,084) or by messages and the RDONE (8 or
    16: 207 k + 8 a = 4,000), and the same with one partition more, where
    the last entry opens an mbuf of its own"""
    cs = []
    for k_, a in ((4, 407), (12, 200)):
        assert 207 * k_ + 8 * a == 4084
        cs.append((f"msgs_fill_{k_}", clients(filling(k_, a), 0, 1, 1), 20, kw(), 2, 12 + 84))
        last = len(filling(k_, a, 1)[-1])
        cs.append((f"msgs_over_{k_}", clients(filling(k_, a, 1), 0, 1, 1), 20, kw(), 2, 12 + last + 84))
    for k_, a in ((8, 293), (16, 86)):
        assert 207 * k_ + 8 * a == 4000
        cs.append((f"rdone_fills_{k_}", clients(filling(k_, a), 0, 1, 1), 21, kw(), 1, 4096))
        cs.append((f"rdone_alone_{k_}", clients(filling(k_, a, 1), 0, 1, 1), 21, kw(), 2, 12 + 84))
    return cs


def malformed_cases():
    """[(name, mbufs, kw, n_taken, stamped)]: one malformed mbuf, as the first
    and as the last of a queue; stamped: the same mbuf with batch id 5 in every
    message, as a sequencer would forward it (None where the rule is the
    client mbuf's own and not the message's)"""
    t = tp(num_wh=4, dist=10, cust=3000, items=1000, part_cnt=2)
    k = kw(node_id=0, node_cnt=2, part_cnt=2, tp_=t)
    good = lambda src=2, n=3: W.batches(0, src, [payment(1 + i, 2, cst=i) for i in range(n)])[0]  # noqa: E731

    def mb(msgs, src=2, cnt=None, cut=lambda b: b):
        """(the client mbuf, the same with the messages stamped)"""
        head = struct.pack("<III", 0, src, len(msgs) if cnt is None else cnt)
        return cut(head + b"".join(msgs)), cut(head + b"".join(m[:12] + struct.pack("<Q", 5) + m[20:] for m in msgs))

    it = [(5, 2, 3), (6, 1, 4)]
    p, no = payment(1, 2), new_order(1, it)
    n_at = HDR + 24 + 81  # (np = 1: the item count's offset)
    bad = {
        "w_id_zero": payment(0), "w_id_over": payment(5), "no_w_id_over": new_order(5, it),
        "d_id_zero": payment(1, d_id=0), "d_id_over": new_order(1, it, d_id=11),
        "c_w_id_over": payment(1, 5), "c_d_id_over": payment(1, 2, c_d_id=11),
        "c_id_zero": payment(1, 2, c_id=0), "c_id_over": new_order(1, it, c_id=3001),
        "type_zero": payment(1, 2, txn_type=0), "type_three": new_order(1, it, txn_type=3),
        "no_without_items": new_order(1, []), "ol_cnt_below_n": new_order(1, it, ol_cnt=1),
        "ol_cnt_above_n": new_order(1, it, ol_cnt=3),
        "item_id_zero": new_order(1, [(0, 1, 1)]), "item_id_over": new_order(1, it + [(1001, 1, 1)]),
        "supply_zero": new_order(1, [(5, 0, 1)]), "supply_over": new_order(1, [(5, 5, 1)] + it),
        "quantity_huge": new_order(1, it + [(5, 1, OPERAND)]),
        "items_63": no[:n_at] + struct.pack("<Q", 63) + b"".join(struct.pack("<3Q", 1, 1, 1) for _ in range(63))
        + struct.pack("<??QQ", False, False, 63, 0),
        "items_huge": no[:n_at] + struct.pack("<Q", (1 << 61) + 2) + no[n_at + 8:],
        "name_without_nul": payment(1, 2, by_last_name=True, c_last=b"ABCDEFGHIJKLMNOP", c_id=0),
        "h_amount_huge": payment(1, 2, h_amount=OPERAND),
        "partition_at_part_cnt": payment(1, 2, parts=[0, 2]),
        "np_65": p[:HDR + 8] + struct.pack("<Q", 65) + bytes(8 * 65) + p[HDR + 24:],
        "np_huge": p[:HDR + 8] + struct.pack("<Q", (1 << 61) + 2) + p[HDR + 16:],
        "rtype": struct.pack("<I", W.CL_RSP) + p[4:],
    }
    assert len(bad["items_63"]) == size(1, 63) and len(bad["np_65"]) == size(65, 0)
    bad = {n: mb([p, m, no]) for n, m in bad.items()}
    bad.update({"truncated_tail": mb([no, p], cut=lambda b: b[:-1]), "truncated_tail_no": mb([p, no], cut=lambda b: b[:-1]),
                "trailing": mb([p, no], cut=lambda b: b + b"\0"), "count_more": mb([p, no], cnt=3),
                "short": (b"\0" * 11, b"\0" * 11),
                "rdone_inside": (mb([p, W.rdone(5)])[0], None), "src_server": (mb([p], src=1)[0], None)})
    out = []
    for name, (b, stamped) in bad.items():
        out.append((name + "_first", [b, good()], k, 0, stamped))
        out.append((name + "_last", [good(), good(3, 2), b], k, 2, stamped))
    # accepted: a Payment carries what it likes in its items and its ol_cnt; a by-name Payment any c_id
    odd, odd_stamped = mb([payment(1, 2, items=[(0, 99, OPERAND)] * 3, ol_cnt=17), no,
                           payment(2, 1, by_last_name=True, c_last=b"ABCDEFGHIJKLMNO", c_id=0)])
    out.append(("payment_items_unchecked", [good(), odd], k, 2, odd_stamped))
    return out
