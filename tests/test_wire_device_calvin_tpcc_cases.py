"""The cases of the CALVIN TPC-C device wire ingress
(dv_wire_ingest_device_calvin_tpcc), checked here on the HOST decoder alone:
every mbuf the GPU tests (tests/test_wire_device_calvin_tpcc.py) call good is
accepted by dv_wire_open under a calvin = 1, DV_TPCC cfg, every one they call
malformed is refused by it, and where the model below says a stream stops is
where dv_wire_decode_batches stops, with the host arrays taken over exactly the
taken messages (repack).  So the GPU tests never compare the device path
against a case its reference would not handle as assumed.  Also the C ABI's
argument checks that need no device.

Layout (tests/wire_fmt.py): under CALVIN the message header is 84 bytes
(batch_id after txn_id) and the fixed part 100; an RDONE is the header alone, a
TPC-C CL_QRY of p partitions and n items 207 + 8 p + 24 n bytes (100, the
partitions, body 89 + 24 n + 18).  A 4,096-byte mbuf holds at most 48 messages
(48 RDONEs: 4,044 bytes) and at most 19 txns; a Payment expands to 3 accesses,
a NewOrder to 3 + 2 ol_cnt, 127 at most.

The YCSB model's parser (test_wire_device_calvin_cases.parse_mbuf) is
module-level there, so parse_mbuf, model and repack are this file's own, written
for this layout.  The query builders (pay, neworder, _items) and the parameter
sets are the TPC-C client cases'.
"""
import ctypes
import struct

import numpy as np
import pytest

import wire_fmt as W
import test_wire_device_calvin_cases as CC
import test_wire_device_tpcc_cases as CT
from dvcc import _lib as L
from dvcc.wire import WireIngress

NODE, NODE_CNT, PART_CNT = CT.NODE, CT.NODE_CNT, CT.PART_CNT
PSETS = CT.PSETS
U64 = (1 << 64) - 1
HDR, FIXED, BODY, TAIL = 84, 100, 89, 18
END, BATCH, CAPACITY, WINDOW, MALFORMED, STALE = range(6)
MAX_TXN_CAP = 1 << 23  # dv_wire_tpcc_dev_out::max_txn's upper bound (include/dvcc.h)
pay, neworder, _items = CT.pay, CT.neworder, CT._items
rdone, mbuf, stream = CC.rdone, CC.mbuf, CC.stream


def tmsg(q, bid, cst=0, txn_id=0, rng=None, patch=None, item_patch=None):
    """One TPC-C CL_QRY of batch bid from wire_fmt.tpcc_query; mq_time and the
    latencies random when rng is given (the decoders skip them); then fields
    overwritten in place: patch {field: value} (rtype, np, a body or tail
    field; 1-byte fields take a byte), item_patch (index, column, value)."""
    b = bytearray(W.tpcc_query(q, cst, txn_id, bid))
    if rng is not None:
        b[20:84] = bytes(rng.integers(0, 256, 64, dtype=np.uint8))
    body = FIXED + 8 * len(q.get("parts", []))
    tail = body + BODY + 24 * len(q.get("items", []))
    for k, v in (patch or {}).items():
        if k == "rtype":
            struct.pack_into("<I", b, 0, v)
        elif k == "np":
            struct.pack_into("<Q", b, HDR + 8, v)
        elif k == "c_last":
            b[body + 56:body + 72] = v
        elif k == "by_last_name":
            b[body + 80] = v
        elif k in ("rbk", "remote"):
            b[tail + CT.TAIL[k]] = v
        elif k in CT.TAIL:
            struct.pack_into("<Q", b, tail + CT.TAIL[k], v)
        else:
            struct.pack_into("<Q", b, body + CT.BODY[k], v)
    if item_patch is not None:
        i, col, v = item_patch
        struct.pack_into("<Q", b, body + BODY + 24 * i + 8 * col, v)
    return bytes(b)


def _acc(q):
    return 3 if q["txn_type"] == 1 else 3 + 2 * len(q["items"])


def parse_mbuf(b):
    """[(offset, size, rtype, batch id, accesses it expands to)] of a well-formed mbuf's messages"""
    cnt = struct.unpack_from("<I", b, 8)[0]
    off, out = 12, []
    for _ in range(cnt):
        rtype, _tid, bid = struct.unpack_from("<IQQ", b, off)
        end, acc = off + HDR, 0
        if rtype == W.CL_QRY:
            npart = struct.unpack_from("<Q", b, off + HDR + 8)[0]
            bo = off + FIXED + 8 * npart
            tt, n = struct.unpack_from("<Q", b, bo)[0], struct.unpack_from("<Q", b, bo + 81)[0]
            end = bo + BODY + 24 * n + TAIL
            acc = 3 if tt == 1 else 3 + 2 * n
        else:
            assert rtype == W.RDONE
        out.append((off, end - off, rtype, bid, acc))
        off = end
    assert off == len(b)
    return out


def model(mbufs, bad, cur=(0, 0), E=None, n_txn=0, n_acc=0, max_txn=1 << 20, max_acc=1 << 24):
    """The header's semantics over mbufs (bytes; those whose index is in `bad`
    are malformed and never parsed): (stop, cursor, E, taken, txns, accesses,
    rdones, longest txn), taken = [(mbuf, first message, end message)], the
    counts the call's own."""
    b, m = cur
    taken, t_all, a_all, r_all, mx = [], 0, 0, 0, 0
    while True:
        if b == len(mbufs):
            return END, (b, 0), E, taken, t_all, a_all, r_all, mx
        ms = None if b in bad else parse_mbuf(mbufs[b])
        if ms is None or m >= len(ms):
            return MALFORMED, (b, m), E, taken, t_all, a_all, r_all, mx
        e = ms[m][3] if E is None else E
        k = m
        while k < len(ms) and ms[k][3] == e:
            k += 1
        t = sum(1 for x in ms[m:k] if x[2] == W.CL_QRY)
        a = sum(x[4] for x in ms[m:k])
        if n_txn + t_all + t > max_txn or n_acc + a_all + a > max_acc:
            return CAPACITY, (b, m), E, taken, t_all, a_all, r_all, mx
        if k > m:
            E = e
            taken.append((b, m, k))
            mx = max([mx] + [x[4] for x in ms[m:k]])
        t_all, a_all, r_all = t_all + t, a_all + a, r_all + sum(1 for x in ms[m:k] if x[2] == W.RDONE)
        if k < len(ms):
            return (BATCH if ms[k][3] > e else STALE), (b, k), E, taken, t_all, a_all, r_all, mx
        b, m = b + 1, 0


def repack(mbufs, taken):
    """the taken messages alone, each mbuf's share an mbuf of its own (same src)"""
    out = []
    for b, m, k in taken:
        ms = parse_mbuf(mbufs[b])
        src = struct.unpack_from("<I", mbufs[b], 4)[0]
        out.append(mbuf([mbufs[b][o:o + sz] for o, sz, *_ in ms[m:k]], src))
    return out


def wire_cfg(pset="base", **kw):
    d = dict(workload=L.TPCC, calvin=1, node_id=NODE, node_cnt=NODE_CNT, part_cnt=PART_CNT, max_req=0,
             synth_table_size=0, tpcc=ctypes.pointer(PSETS[pset]) if pset else None)
    d.update(kw)
    return L.WireCfg(**d)


def _ingress(pset):
    return WireIngress(L.TPCC, 1 << 16, 1 << 20, node_id=NODE, node_cnt=NODE_CNT, part_cnt=PART_CNT, calvin=True,
                       tpcc=PSETS[pset])


def host_decode(mbufs, pset="base"):
    """mbufs of one batch id through the host decoder with ample capacity: one epoch (WireEpoch)"""
    w = _ingress(pset)
    if mbufs:
        buf, off = stream(mbufs)
        assert w.feed_buffer(buf, off) == []
    return w.take()


def host_stop(mbufs, cur=(0, 0), E=None, pset="base"):
    """dv_wire_decode_batches from the cursor with ample capacity: (stop,
    cursor, txns, accesses, rdones, batch id); the first mbuf trimmed to its
    messages from the cursor (the host cursor cannot skip)"""
    b0, m0 = cur
    first = []
    if b0 < len(mbufs):
        ms = parse_mbuf(mbufs[b0])
        first = [mbuf([mbufs[b0][o:o + sz] for o, sz, *_ in ms[m0:]], struct.unpack_from("<I", mbufs[b0], 4)[0])]
    rest = first + list(mbufs[b0 + 1:])
    w = _ingress(pset)
    if E is not None:
        w.ep.batch_id = E
    if not rest:
        return END, (b0, 0), 0, 0, 0, E
    buf, off = stream(rest)
    c, nxt = L.WireCursor(), ctypes.c_uint32(0)
    rc = L.lib().dv_wire_decode_batches(ctypes.byref(w.cfg), buf.ctypes.data_as(ctypes.c_void_p),
                                        off.ctypes.data_as(ctypes.c_void_p), len(rest), ctypes.byref(c),
                                        ctypes.byref(nxt), ctypes.byref(w.ep))
    e = w.ep
    bid = None if e.batch_id == U64 else int(e.batch_id)
    if rc == L.DV_OK:
        return END, (len(mbufs), 0), e.n_txn, e.n_acc, e.rdone, bid
    j = nxt.value - 1  # the mbuf the cursor stands in
    cnt = struct.unpack_from("<I", rest[j], 8)[0]
    at = (b0 + j, cnt - c.left + (m0 if j == 0 else 0))
    return (BATCH if rc == L.WIRE_MORE else STALE), at, e.n_txn, e.n_acc, e.rdone, bid


# ---- the cases
def shape_queries(rng, p):
    """[(name, query, tmsg kwargs)]: every message shape the issue names"""
    W_ = p.num_wh
    junk = U64 - 2
    out = [("pay_by_id", pay(W_, 10, 1000, c_w=1, c_d=1, h=(1 << 56) - 1), {}),
           ("pay_name_0", pay(2, 3, 0, name=b""), {}),
           ("pay_name_1", pay(2, 3, 0, c_w=W_, c_d=7, name=b"A"), {}),
           ("pay_name_15", pay(1, 1, 0, name=b"ABCDEFGHIJKLMNO"), {}),
           ("pay_name_garbage_after_nul", pay(3, 4, 0, name=b"BAR"),
            dict(patch=dict(c_last=b"BAR\0junk\xff\x80junk!!"))),
           ("pay_name_odd_bytes", pay(3, 4, 0, c_w=W_, name=b"@\x80\xffA0z"), {}),
           ("pay_by_last_name_byte_2", pay(1, 2, 0, name=b"OUGHTPRI"), dict(patch=dict(by_last_name=2))),
           ("pay_with_3_garbage_items",
            pay(1, 2, 5, items=[(0, 0, 1 << 60), (junk, junk, junk), (1 << 32, 1 << 33, 0)]), {}),
           ("pay_by_id_unchecked_garbage",
            pay(1, 2, 5, d_w_id=junk, c_last=b"\xff" * 16, ol_cnt=junk, o_entry_d=junk),
            dict(patch=dict(rbk=0xEE, remote=0x7F))),
           ("pay_by_name_unchecked_garbage", pay(1, 2, junk, name=b"ESE", d_w_id=0, ol_cnt=63),
            dict(patch=dict(rbk=2)))]
    for n in (1, 5, 15, 62):
        out.append((f"neworder_{n}", neworder(_items(rng, n, p, 2), 2, 9, 999), {}))
    out.append(("neworder_unchecked_garbage",
                neworder(_items(rng, 4, p, 1), W_, 1, 1, d_w_id=junk, c_w_id=junk, c_d_id=0, c_last=b"\x80" * 16,
                         h_amount=junk, by_last_name=True, o_entry_d=junk),
                dict(patch=dict(rbk=9, remote=0xFF, by_last_name=0xCC))))
    for k in (0, 1, 4, 64):
        out.append((f"partitions_{k}", pay(1, 1, 1, parts=[i % PART_CNT for i in range(k)]), {}))
        out.append((f"neworder_partitions_{k}",
                    neworder(_items(rng, 2, p, 1), parts=[(i + 1) % PART_CNT for i in range(k)]), {}))
    return out


def good_cases(pset="base", seed=7, bid=9):
    """[(name, mbuf bytes, txns, accesses, rdones)] under PSETS[pset], all of
    batch `bid`, garbage in the latency fields"""
    rng = np.random.default_rng(seed)
    p = PSETS[pset]
    W_ = p.num_wh
    out = []
    tid = iter(range(1, 10_000))
    t = lambda q, **kw: tmsg(q, bid, 500 + next(tid), 3 * next(tid), rng, **kw)  # noqa: E731
    # the shapes, packed as MessageThread packs them, an RDONE between every third pair
    msgs, accs = [], []
    for i, (name, q, kw) in enumerate(shape_queries(rng, p)):
        msgs.append(t(q, **kw))
        accs.append(_acc(q))
        if i % 3 == 2:
            msgs.append(rdone(bid, rng))
            accs.append(None)
    pos = 0
    for b in W.batches(NODE, 5, msgs):
        cnt = struct.unpack_from("<I", b, 8)[0]
        mine = accs[pos:pos + cnt]
        out.append((f"shapes{pos}", b, sum(1 for a in mine if a is not None), sum(a or 0 for a in mine),
                    sum(1 for a in mine if a is None)))
        pos += cnt
    out.append(("nineteen_payments", mbuf([t(pay(1 + i % W_, 1 + i % 10, 1 + i, parts=())) for i in range(19)], 7),
                19, 57, 0))
    assert len(out[-1][1]) == 12 + 19 * 207 and 12 + 20 * 207 > 4096
    b48 = mbuf([rdone(bid, rng) for _ in range(48)], 7)
    assert len(b48) == 4044
    out.append(("rdones_48", b48, 0, 0, 48))
    # exactly 4,096 bytes, an RDONE last: 12 + 2 x 84 + 4 x 207 + 8 x 2 + 24 x (62 + 62 + 4)
    qs = [neworder(_items(rng, 62, p, 1), parts=()), pay(2, 2, 2, parts=(0, 3)),
          neworder(_items(rng, 62, p, W_), W_, parts=()), neworder(_items(rng, 4, p, 1), parts=())]
    full = mbuf([t(qs[0]), t(qs[1]), rdone(bid, rng), t(qs[2]), t(qs[3]), rdone(bid, rng)], 8)
    assert len(full) == 4096
    out.append(("full_4096_rdone_last", full, 4, sum(_acc(q) for q in qs), 2))
    # an RDONE directly in front of a CL_QRY: read at body offsets from the RDONE (np at +92, ids from +100 on), the
    # query's txn_id / batch id words and its random latencies are out-of-range ids
    trap = mbuf([rdone(bid, rng), tmsg(pay(1, 1, 1), bid, 7, U64 - 5, rng), rdone(bid, rng),
                 tmsg(neworder(_items(rng, 3, p, 1)), bid, 8, 1 << 40, rng)], 6)
    out.append(("rdone_in_front_of_a_query", trap, 2, 12, 2))
    # past lane 64 of the flat loops: 72 partitions in an mbuf, 80 items in an mbuf, an RDONE behind each
    qs = [pay(1 + i % W_, 1 + i % 10, 1 + i, parts=[i % PART_CNT, 1, 2, 3]) for i in range(16)]
    out.append(("partitions_64", mbuf([t(q) for q in qs] + [rdone(bid, rng)], 9), 16, 48, 1))
    assert len(out[-1][1]) == 16 * 239 + 84 + 12 == 3920
    qs = [neworder(_items(rng, 40, p, 1)), neworder(_items(rng, 40, p, 2), 2)]
    out.append(("items_80", mbuf([t(qs[0]), rdone(bid, rng), t(qs[1])], 9), 2, 166, 1))
    return out


def _ok_msgs(rng, p, n, bid):
    qs = CT._ok_msgs(rng, p, n)
    return [tmsg(x, bid, 40 + i, 7 + i, rng) for i, x in enumerate(qs)]


def malformed_kinds(seed=11):
    """[(name, query or None, kwargs of tmsg)] under PSETS['base']: the TPC-C
    client cases' kinds of bad message (test_wire_device_tpcc_cases), item
    cases as item=(column, value); a None query is the kind's own bytes"""
    rng = np.random.default_rng(seed)
    p = PSETS["base"]
    big = (1 << 32) + 1
    kinds = []
    for v in (0, 3, big):
        kinds.append((f"txn_type_{v}", pay(), dict(patch=dict(txn_type=v))))
    rng_fields = [("pay", "w_id", p.num_wh), ("pay", "c_w_id", p.num_wh), ("pay", "d_id", p.dist_per_wh),
                  ("pay", "c_d_id", p.dist_per_wh), ("pay", "c_id", p.cust_per_dist), ("no", "w_id", p.num_wh),
                  ("no", "d_id", p.dist_per_wh), ("no", "c_id", p.cust_per_dist)]
    for who, f, bound in rng_fields:
        for v in (0, bound + 1, big):
            q = pay(2, 2, 2) if who == "pay" else neworder(_items(rng, 3, p, 1))
            kinds.append((f"{who}_{f}_{v}", q, dict(patch={f: v})))
    for col, f, bound in ((0, "ol_i_id", p.max_items), (1, "ol_supply_w_id", p.num_wh)):
        for v in (0, bound + 1, big):
            kinds.append((f"item_{f}_{v}", neworder(_items(rng, 5, p, 1)), dict(item=(col, v))))
    kinds.append(("item_ol_quantity_2_56", neworder(_items(rng, 5, p, 1)), dict(item=(2, 1 << 56))))
    kinds.append(("pay_name_without_nul", pay(1, 1, 0, name=b"ABCDEFGHIJKLMNOP"), {}))
    kinds.append(("pay_h_amount_2_56", pay(h=1 << 56), {}))
    kinds.append(("neworder_ol_cnt_0", neworder([]), {}))
    kinds.append(("neworder_ol_cnt_above_n", neworder(_items(rng, 4, p, 1)), dict(patch=dict(ol_cnt=5))))
    kinds.append(("neworder_ol_cnt_below_n", neworder(_items(rng, 4, p, 1)), dict(patch=dict(ol_cnt=3))))
    kinds.append(("neworder_ol_cnt_high_bits", neworder(_items(rng, 4, p, 1)), dict(patch=dict(ol_cnt=(1 << 32) + 4))))
    kinds.append(("items_63", neworder([(1 + i, 1, 1) for i in range(63)]), {}))
    kinds.append(("pay_items_63", pay(items=[(1 + i, 1, 1) for i in range(63)]), {}))
    kinds.append(("items_wrap_2_61_plus_1", neworder(_items(rng, 1, p, 1)), dict(patch=dict(n=(1 << 61) + 1))))
    kinds.append(("items_2_32_plus_1", pay(items=[(1, 1, 1)]), dict(patch=dict(n=big))))
    kinds.append(("partition_is_part_cnt", pay(parts=(0, PART_CNT, 1)), {}))
    kinds.append(("partitions_65", pay(parts=[0] * 65), {}))
    kinds.append(("partitions_wrap_2_61", pay(parts=()), dict(patch=dict(np=1 << 61))))
    kinds.append(("rtype_cl_rsp", pay(), dict(patch=dict(rtype=W.CL_RSP))))
    kinds.append(("rtype_rdone_shaped_like_a_query", pay(), dict(patch=dict(rtype=W.RDONE))))
    # CALVIN's own (an RDONE alone is a message here: the client cases' rtype_rdone is well-formed)
    kinds.append(("unknown_rtype", None, dict(raw=lambda bid, rng: CC.header(7, 1, bid, rng))))
    kinds.append(("batch_id_max_on_a_query", None, dict(raw=lambda bid, rng: tmsg(pay(), U64, 1, 6, rng))))
    kinds.append(("batch_id_max_on_an_rdone", None, dict(raw=lambda bid, rng: rdone(U64, rng))))
    kinds.append(("truncated_rdone", None, dict(raw=lambda bid, rng: rdone(bid, rng)[:-8])))
    kinds.append(("rdone_with_trailing_bytes", None, dict(raw=lambda bid, rng: rdone(bid, rng) + b"\0" * 8)))
    return kinds


def bad_message(kind, where, bid, rng):
    """the kind's bad message of batch bid; where 0 / 2 / 4 also places a bad item first / middle / last of its list"""
    name, q, kw = kind
    kw = dict(kw)
    if "raw" in kw:
        return kw["raw"](bid, rng)
    if "item" in kw:
        col, v = kw.pop("item")
        kw["item_patch"] = ({0: 0, 2: len(q["items"]) // 2, 4: len(q["items"]) - 1}[where], col, v)
    return tmsg(q, bid, 9, 5, rng, **kw)


def malformed_mbuf(kind, where, bid=9, seed=12):
    """a five-message mbuf of batch bid, the kind's bad message at place `where` (0, 2, 4)"""
    rng = np.random.default_rng(seed)
    msgs = _ok_msgs(rng, PSETS["base"], 5, bid)
    msgs[where] = bad_message(kind, where, bid, rng)
    return mbuf(msgs)


def outside_run_mbufs(kind, bid=9, seed=14):
    """(in front of the cursor, behind the cut): two mbufs whose bad message is
    no part of the run -- message 0 of [bad, ok, ok] read from cursor message
    1, and the message of the next batch behind [ok, RDONE]"""
    rng = np.random.default_rng(seed)
    ok = _ok_msgs(rng, PSETS["base"], 4, bid)
    front = mbuf([bad_message(kind, 2, bid - 1 if "batch_id_max" not in kind[0] else bid, rng), ok[0], ok[1]])
    behind = mbuf([ok[2], rdone(bid, rng), bad_message(kind, 2, bid + 1, rng)])
    return front, behind


def batch_level_cases(seed=13, bid=9):
    """[(name, mbuf bytes)]: the refusals of the mbuf as a whole"""
    rng = np.random.default_rng(seed)
    p = PSETS["base"]
    ok = lambda: _ok_msgs(rng, p, 3, bid)  # noqa: E731
    m = []
    m.append(("len_below_12", struct.pack("<II", NODE, 5)))
    m.append(("one_byte_short", mbuf(ok())[:-1]))
    m.append(("one_byte_over", mbuf(ok()) + b"\0"))
    m.append(("count_one_more", mbuf(ok(), count=4)))
    m.append(("count_one_less", mbuf(ok(), count=2)))
    m.append(("count_zero", mbuf(ok(), count=0)))
    m.append(("count_zero_and_no_bytes", mbuf([], count=0)))
    m.append(("count_huge", mbuf(ok(), count=0xFFFFFFFF)))
    m.append(("dest_not_this_node", mbuf(ok(), dest=NODE + 1)))
    m.append(("src_is_this_node", mbuf(ok(), src=NODE)))
    m.append(("len_above_4096", mbuf([tmsg(neworder(_items(rng, 62, p, 1)), bid) for _ in range(3)])))
    assert len(m[-1][1]) > 4096
    m.append(("forty_nine_rdones", mbuf([rdone(bid, rng) for _ in range(49)])))
    # the bad field past flat index 63 of its loop, and in a NewOrder behind an RDONE and a Payment with items
    parts = [[0, 1, 2, 3] for _ in range(17)]
    parts[66 // 4][66 % 4] = PART_CNT
    m.append(("partition_66_of_68_out_of_range",
              mbuf([tmsg(pay(1, 1, 1 + i, parts=x), bid) for i, x in enumerate(parts)])))
    m.append(("item_70_of_80_i_id_above_max_items",
              mbuf([tmsg(neworder(_items(rng, 40, p, 1)), bid), rdone(bid, rng), tmsg(pay(items=[(0, 0, 0)] * 3), bid),
                    tmsg(neworder(_items(rng, 40, p, 1)), bid, item_patch=(70 - 40, 0, p.max_items + 1))])))
    return m


OFF_CASES = CC.OFF_CASES


def cut_cases(seed=13, e=9):
    """[(name, mbufs, cursor, E or None)]: streams that stop at a batch
    boundary or a stale message, or run to their end"""
    rng = np.random.default_rng(seed)
    p = PSETS["base"]
    tid = iter(range(100, 10_000))

    def q(bid, n=2):  # n items: 0 a Payment
        x = neworder(_items(rng, n, p, 1), 1 + n % p.num_wh) if n else pay(1, 1 + next(tid) % 10, 1 + next(tid) % 1000)
        return tmsg(x, bid, 500 + n, next(tid), rng)

    head = [mbuf([q(e, 3), q(e, 0)], 5), mbuf([q(e, 1)], 6)]
    out = []
    out.append(("cut_at_message_1", head + [mbuf([rdone(e, rng), q(e + 1), q(e + 1)], 5), mbuf([q(e + 1)], 5)],
                (0, 0), None))
    out.append(("cut_at_a_middle_message",
                head + [mbuf([q(e), q(e, 5), rdone(e, rng), q(e + 1), q(e + 1, 4), rdone(e + 1, rng)], 5)], (0, 0), e))
    out.append(("cut_at_the_last_message", head + [mbuf([q(e), q(e, 0), rdone(e, rng), q(e + 2)], 5)], (0, 0), None))
    out.append(("mbuf_wholly_of_the_later_batch", head + [mbuf([q(e + 1), rdone(e + 1, rng)], 5)], (0, 0), None))
    out.append(("first_message_already_later", [mbuf([q(e + 1), q(e + 1, 0)], 5)] + head, (0, 0), e))
    out.append(("E_from_a_cursor_inside_an_mbuf",
                [mbuf([q(e - 1), rdone(e - 1, rng), q(e, 0), q(e, 4)], 5), mbuf([q(e), rdone(e, rng), q(e + 1)], 6)],
                (0, 2), None))
    out.append(("cursor_at_the_last_message", [mbuf([q(e - 1), q(e)], 5), mbuf([rdone(e, rng)], 5)], (0, 1), None))
    out.append(("runs_to_the_end", head + [mbuf([q(e), rdone(e, rng)], 5)], (0, 0), e))
    out.append(("nothing_left", head, (2, 0), e))
    out.append(("stale_at_an_mbufs_first_message", head + [mbuf([q(e - 1), q(e)], 5)], (0, 0), None))
    out.append(("stale_mid_mbuf", head + [mbuf([q(e, 0), q(e, 4), q(e - 3), q(e)], 5)], (0, 0), e))
    out.append(("stale_at_the_cursor", [mbuf([q(e - 1), q(e)], 5)], (0, 0), e))
    # where the run's access sum and the whole mbuf's item sum differ: a 62-item NewOrder on either side of the cut
    out.append(("neworder_62_in_front_of_the_cut", head + [mbuf([q(e, 0), q(e, 62), q(e + 1, 2), q(e + 1, 0)], 5)],
                (0, 0), None))
    out.append(("neworder_62_behind_the_cut", head + [mbuf([q(e, 2), q(e, 0), q(e + 1, 62), q(e + 1, 1)], 5)],
                (0, 0), e))
    out.append(("neworder_62_on_both_sides", [mbuf([q(e - 1, 62), q(e, 1), q(e, 0), rdone(e, rng), q(e + 1, 62)], 5)],
                (0, 1), None))
    return out


# ---- on the host decoder alone
def _open(b, pset="base"):
    cfg = wire_cfg(pset)
    buf = np.frombuffer(b, np.uint8)
    cur = L.WireCursor()
    return L.lib().dv_wire_open(ctypes.byref(cfg), buf.ctypes.data_as(ctypes.c_void_p), len(buf), ctypes.byref(cur))


@pytest.mark.parametrize("pset", list(PSETS))
def test_good_cases_are_accepted_with_the_expected_counts(pset):
    cases = good_cases(pset)
    assert {c[0] for c in cases} >= {"nineteen_payments", "rdones_48", "full_4096_rdone_last",
                                     "rdone_in_front_of_a_query"}
    lens, tables = set(), set()
    for name, b, txns, accs, rd in cases:
        assert _open(b, pset) == L.DV_OK, name
        ep = host_decode([b], pset)
        assert (ep.n_txn, ep.n_acc, ep.rdone, ep.batch_id) == (txns, accs, rd, 9), name
        ms = parse_mbuf(b)
        assert (sum(1 for x in ms if x[2] == W.CL_QRY), sum(x[4] for x in ms)) == (txns, accs), name
        assert (np.diff(ep.txn_begin.astype(np.int64)) == [x[4] for x in ms if x[2] == W.CL_QRY]).all(), name
        lens |= set(np.diff(ep.txn_begin.astype(np.int64)).tolist())
        tables |= set(ep.tables.tolist())
    assert lens >= {3, 5, 13, 33, 127} and tables == {0, 1, 2, 3, 4, 5}
    assert max(len(c[1]) for c in cases) == 4096 and parse_mbuf(cases[-1][1])


def test_the_full_mbuf_ends_in_an_rdone_and_the_trap_reads_as_bad_ids():
    cases = dict((c[0], c[1]) for c in good_cases())
    ms = parse_mbuf(cases["full_4096_rdone_last"])
    assert ms[-1][2] == W.RDONE and ms[-1][0] + HDR == 4096
    b = cases["rdone_in_front_of_a_query"]
    ms = parse_mbuf(b)
    assert [x[2] for x in ms] == [W.RDONE, W.CL_QRY, W.RDONE, W.CL_QRY]
    p = PSETS["base"]
    for o in (ms[0][0], ms[2][0]):  # w_id / d_id read at the body offset a query of no partitions would have
        w, d = struct.unpack_from("<QQ", b, o + FIXED + 8)
        assert not (1 <= w <= p.num_wh and 1 <= d <= p.dist_per_wh)


@pytest.mark.parametrize("kind", malformed_kinds(), ids=lambda k: k[0])
def test_malformed_kinds_are_refused_by_the_host_decoder(kind):
    for where in (0, 2, 4):
        assert _open(malformed_mbuf(kind, where)) == L.DV_ERR_ARG
    front, behind = outside_run_mbufs(kind)
    assert _open(front) == L.DV_ERR_ARG and _open(behind) == L.DV_ERR_ARG


def test_every_tpcc_malformed_kind_is_re_encoded():
    mine = {k[0] for k in malformed_kinds()}
    theirs = {c[0].rsplit("_", 1)[0] for c in CT.malformed_cases()
              if c[0].rsplit("_", 1)[1] in ("first", "middle", "last")}
    assert theirs - mine == {"rtype_rdone"}  # (an RDONE is a message under CALVIN)
    assert mine >= {"unknown_rtype", "batch_id_max_on_a_query", "batch_id_max_on_an_rdone", "truncated_rdone"}


@pytest.mark.parametrize("case", batch_level_cases(), ids=lambda c: c[0])
def test_batch_level_cases_are_refused_by_the_host_decoder(case):
    assert _open(case[1]) == L.DV_ERR_ARG


def test_malformed_mbufs_differ_from_a_good_one_only_where_named():
    rng = np.random.default_rng(12)
    p = PSETS["base"]
    assert _open(mbuf(_ok_msgs(rng, p, 5, 9))) == L.DV_OK
    ok = _ok_msgs(rng, p, 4, 9)
    assert _open(mbuf([tmsg(pay(), 8, 1, 6, rng), ok[0], ok[1]])) == L.DV_OK
    assert _open(mbuf([ok[2], rdone(9, rng), tmsg(pay(), 10, 1, 6, rng)])) == L.DV_OK
    assert _open(mbuf([tmsg(neworder(_items(rng, 5, p, 1)), 9, item_patch=(2, 2, (1 << 56) - 1))])) == L.DV_OK
    assert _open(mbuf([tmsg(neworder([(1 + i, 1, 1) for i in range(62)]), 9)])) == L.DV_OK
    # the last batch-level case without its patch
    assert _open(mbuf([tmsg(neworder(_items(rng, 40, p, 1)), 9), rdone(9, rng), tmsg(pay(items=[(0, 0, 0)] * 3), 9),
                       tmsg(neworder(_items(rng, 40, p, 1)), 9)])) == L.DV_OK


@pytest.mark.parametrize("case", cut_cases(), ids=lambda c: c[0])
def test_the_model_stops_where_the_host_decoder_stops(case):
    name, mbufs, cur, E = case
    for b in mbufs:
        assert _open(b) == L.DV_OK
    stop, at, e_out, taken, t, a, r, mx = model(mbufs, set(), cur, E)
    h_stop, h_at, h_t, h_a, h_r, h_e = host_stop(mbufs, cur, E)
    assert (stop, at, t, a, r) == (h_stop, h_at, h_t, h_a, h_r)
    assert e_out == h_e or (not taken and h_e == E)
    # ... and the taken messages alone decode to the same epoch
    ref = host_decode(repack(mbufs, taken))
    assert (ref.n_txn, ref.n_acc, ref.rdone) == (t, a, r) and (ref.max_txn_acc() if t else 0) == mx
    if taken:
        assert ref.batch_id == e_out
    # resuming at the cursor reproduces the host decoder's next epoch
    if stop == BATCH:
        stop2, at2, e2, taken2, t2, a2, r2, _ = model(mbufs, set(), at, None)
        assert (stop2, at2, t2, a2, r2, e2) == host_stop(mbufs, at, None)
        assert e2 > (E if e_out is None else e_out)


def test_the_cut_cases_cover_what_the_issue_names():
    got = {c[0]: model(c[1], set(), c[2], c[3]) for c in cut_cases()}
    assert got["cut_at_message_1"][:2] == (BATCH, (2, 1))
    assert got["cut_at_a_middle_message"][:2] == (BATCH, (2, 3))
    assert got["cut_at_the_last_message"][:2] == (BATCH, (2, 3))
    assert got["mbuf_wholly_of_the_later_batch"][:2] == (BATCH, (2, 0))
    assert got["first_message_already_later"][:2] == (BATCH, (0, 0)) and not got["first_message_already_later"][3]
    assert got["E_from_a_cursor_inside_an_mbuf"][:3] == (BATCH, (1, 2), 9)
    assert got["runs_to_the_end"][:2] == (END, (3, 0)) and got["nothing_left"][:2] == (END, (2, 0))
    assert got["stale_at_an_mbufs_first_message"][:2] == (STALE, (2, 0))
    assert got["stale_mid_mbuf"][:2] == (STALE, (2, 2)) and got["stale_mid_mbuf"][4] == 5
    assert got["stale_at_the_cursor"][:2] == (STALE, (0, 0))
    # the run's accesses against the whole mbuf's items: 127 on one side of the cut only
    a, b, c = (got[k] for k in ("neworder_62_in_front_of_the_cut", "neworder_62_behind_the_cut",
                                "neworder_62_on_both_sides"))
    assert a[:2] == (BATCH, (2, 2)) and a[7] == 127 and b[:2] == (BATCH, (2, 2)) and b[7] < 127
    assert c[:2] == (BATCH, (0, 4)) and c[4:8] == (2, 5 + 3, 1, 5)


# ---- the C ABI without a device
def _out(**kw):
    one = 0x1000  # (never dereferenced: every call here is refused before a launch)
    d = dict(max_txn=16, pad_=0, max_acc=160, txn_begin=one, n_acc_dev=None, keys=one, types=one, acc_txn=one,
             tables=one, args=one, txn_type=None, owner=None, txn_id=None, client_startts=None, return_node=None)
    d.update(kw)
    return L.WireTpccDevOut(**d)


def _pos(**kw):
    d = dict(batch=0, msg=0, n_txn=0, rdone=0, n_acc=0, batch_id=U64, max_txn_acc=0, stop=77)
    d.update(kw)
    return L.WireCalvinPos(**d)


def ingest(ctx, cfg, out, pos, buf=0x1000, off=0x1000, n_batches=3):
    return L.lib().dv_wire_ingest_device_calvin_tpcc(ctx, ctypes.byref(cfg) if cfg is not None else None, buf, 64, off,
                                                     n_batches, ctypes.byref(out) if out is not None else None,
                                                     ctypes.byref(pos) if pos is not None else None)


def refused_arguments():
    """[(name, cfg, out, pos)]: argument sets dv_wire_ingest_device_calvin_tpcc
    refuses before any launch, whatever the context (shared with the GPU test,
    which passes a live one); n_batches is 3"""
    bad = lambda **kw: ctypes.pointer(L.TpccParams(**{**dict(  # noqa: E731
        num_wh=4, dist_per_wh=10, cust_per_dist=1000, max_items=2000, max_items_per_txn=15, part_cnt=3,
        part_per_txn=2, wh_update=1, perc_payment=0.5, mpr=1.0), **kw}))
    r = [
        ("not_calvin", wire_cfg(calvin=0), _out(), _pos()),
        ("ycsb", wire_cfg(workload=L.YCSB), _out(), _pos()),
        ("no_params", wire_cfg(None), _out(), _pos()),
        ("params_cust_per_dist_999", wire_cfg(tpcc=bad(cust_per_dist=999)), _out(), _pos()),
        ("params_part_cnt_above_num_wh", wire_cfg(tpcc=bad(part_cnt=5)), _out(), _pos()),
        ("params_no_warehouse", wire_cfg(tpcc=bad(num_wh=0, part_cnt=0)), _out(), _pos()),
        ("params_items_per_txn_63", wire_cfg(tpcc=bad(max_items_per_txn=63)), _out(), _pos()),
        ("part_cnt_zero", wire_cfg(part_cnt=0), _out(), _pos()),
        ("node_cnt_zero", wire_cfg(node_cnt=0), _out(), _pos()),
        ("max_txn_zero", wire_cfg(), _out(max_txn=0), _pos()),
        ("max_txn_above_2_23", wire_cfg(), _out(max_txn=MAX_TXN_CAP + 1), _pos()),
        ("max_acc_2_32", wire_cfg(), _out(max_acc=1 << 32), _pos()),
        ("cursor_past_the_stream", wire_cfg(), _out(), _pos(batch=4)),
        ("message_cursor_at_the_end", wire_cfg(), _out(), _pos(batch=3, msg=1)),
        ("n_txn_above_max_txn", wire_cfg(), _out(), _pos(n_txn=17)),
        ("n_acc_above_max_acc", wire_cfg(), _out(), _pos(n_acc=161)),
    ]
    for f in ("txn_begin", "keys", "types", "acc_txn", "tables", "args"):
        r.append((f"no_{f}", wire_cfg(), _out(**{f: None}), _pos()))
    return r


def test_the_new_entry_rejects_null_and_unsupported_arguments():
    """DV_ERR_ARG before any device is touched, *pos as it was"""
    assert ingest(None, wire_cfg(), _out(), _pos()) == L.DV_ERR_ARG
    assert ingest(None, None, None, None, 0, 0) == L.DV_ERR_ARG
    p = _pos()
    assert ingest(None, wire_cfg(), _out(), p, buf=0) == L.DV_ERR_ARG
    assert ingest(None, wire_cfg(), _out(), p, off=0) == L.DV_ERR_ARG and bytes(p) == bytes(_pos())
    for name, c, o, p in refused_arguments():
        before = bytes(p)
        assert ingest(None, c, o, p) == L.DV_ERR_ARG, name
        assert bytes(p) == before, name


def test_the_existing_entries_refuse_what_they_refused():
    cfg = wire_cfg()
    r = L.WireDevResult(status=77)
    y = CC._out()
    assert L.lib().dv_wire_ingest_device(None, ctypes.byref(cfg), 0x1000, 64, 0x1000, 1, 0, ctypes.byref(y), 0,
                                         ctypes.byref(r)) == L.DV_ERR_ARG
    t = CT._out()
    assert L.lib().dv_wire_ingest_device_tpcc(None, ctypes.byref(cfg), 0x1000, 64, 0x1000, 1, 0, ctypes.byref(t), 0,
                                              ctypes.byref(r)) == L.DV_ERR_ARG
    p = CC._pos()
    assert CC.ingest(None, cfg, y, p) == L.DV_ERR_ARG and r.status == 77 and bytes(p) == bytes(CC._pos())
