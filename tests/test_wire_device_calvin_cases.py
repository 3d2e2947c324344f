"""The cases of the CALVIN device wire ingress (dv_wire_ingest_device_calvin),
checked here on the HOST decoder alone: every mbuf the GPU tests
(tests/test_wire_device_calvin.py) call good is accepted by dv_wire_open under
a CALVIN cfg, every one they call malformed is refused by it, and where the
model below says a stream stops (at the end, at a later batch, at a stale
message) is where dv_wire_decode_batches stops.  So the GPU tests never compare
the device path against a case its reference would not handle as assumed.
Also the C ABI's argument checks that need no device.

Layout (tests/wire_fmt.py): under CALVIN the message header is 84 bytes
(batch_id after txn_id); an RDONE is the header alone, a YCSB CL_QRY of p
partitions and n requests 108 + 8 p + 24 n bytes.  A 4,096-byte mbuf holds at
most 48 messages (48 RDONEs: 4,044 bytes) and at most 37 txns.

wire_fmt.parse_batch reads reply batches (CL_RSP / CALVIN_ACK) only; the
sequencer streams' own messages are counted by parse_mbuf here, written from
the same field order.
"""
import ctypes
import struct

import numpy as np
import pytest

import wire_fmt as W
import test_wire_device_cases as C0
from dvcc import _lib as L
from dvcc.wire import WireIngress

NODE, NODE_CNT, PART_CNT, ROWS = C0.NODE, C0.NODE_CNT, C0.PART_CNT, C0.ROWS
U64 = (1 << 64) - 1
HDR, FIXED = 84, 100
END, BATCH, CAPACITY, WINDOW, MALFORMED, STALE = range(6)


def header(rtype, txn_id, bid, rng=None):
    """the CALVIN message header; mq_time and the latencies random when rng is
    given (statistics: the decoders skip them)"""
    junk = bytes(rng.integers(0, 256, 64, dtype=np.uint8)) if rng is not None else b"\0" * 64
    return struct.pack("<IQQ", rtype, txn_id, bid) + junk


def message(reqs, parts, bid, cst=0, txn_id=0, rng=None, rtype=W.CL_QRY, n_parts=None, n_reqs=None):
    """One CL_QRY of batch bid: reqs [(acctype, key)], parts [partition]; the
    requests' padding and value bytes random when rng is given; n_parts /
    n_reqs: the counts written, when they are to lie."""
    body = b""
    for a, k in reqs:
        junk = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) if rng is not None else b"\x5a" * 12
        body += struct.pack("<I", a) + junk[:4] + struct.pack("<Q", k) + junk[4:]
    return (header(rtype, txn_id, bid, rng) + struct.pack("<QQ", cst, len(parts) if n_parts is None else n_parts)
            + b"".join(struct.pack("<Q", p) for p in parts)
            + struct.pack("<Q", len(reqs) if n_reqs is None else n_reqs) + body)


def rdone(bid, rng=None):
    return header(W.RDONE, U64, bid, rng)


def mbuf(msgs, src=5, dest=NODE, count=None):
    return struct.pack("<III", dest, src, len(msgs) if count is None else count) + b"".join(msgs)


def _reqs(rng, n):
    return [(int(rng.integers(0, 2)), int(rng.integers(0, ROWS))) for _ in range(n)]


def parse_mbuf(b):
    """[(offset, size, rtype, batch id, requests)] of a well-formed mbuf's messages"""
    cnt = struct.unpack_from("<I", b, 8)[0]
    off, out = 12, []
    for _ in range(cnt):
        rtype, _tid, bid = struct.unpack_from("<IQQ", b, off)
        end, n = off + HDR, 0
        if rtype == W.CL_QRY:
            npart = struct.unpack_from("<Q", b, off + HDR + 8)[0]
            n = struct.unpack_from("<Q", b, off + FIXED + 8 * npart)[0]
            end = off + FIXED + 8 * npart + 8 + 24 * n
        else:
            assert rtype == W.RDONE
        out.append((off, end - off, rtype, bid, n))
        off = end
    assert off == len(b)
    return out


def model(mbufs, bad, cur=(0, 0), E=None, n_txn=0, n_acc=0, max_txn=1 << 20, max_acc=1 << 24):
    """The header's semantics over mbufs (bytes; those whose index is in `bad`
    are malformed and never parsed): (stop, cursor, E, taken, txns, accesses,
    rdones), taken = [(mbuf, first message, end message)], the counts the
    call's own."""
    b, m = cur
    taken, t_all, a_all, r_all = [], 0, 0, 0
    while True:
        if b == len(mbufs):
            return END, (b, 0), E, taken, t_all, a_all, r_all
        ms = None if b in bad else parse_mbuf(mbufs[b])
        if ms is None or m >= len(ms):
            return MALFORMED, (b, m), E, taken, t_all, a_all, r_all
        e = ms[m][3] if E is None else E
        k = m
        while k < len(ms) and ms[k][3] == e:
            k += 1
        t = sum(1 for x in ms[m:k] if x[2] == W.CL_QRY)
        a = sum(x[4] for x in ms[m:k])
        if n_txn + t_all + t > max_txn or n_acc + a_all + a > max_acc:
            return CAPACITY, (b, m), E, taken, t_all, a_all, r_all
        if k > m:
            E = e
            taken.append((b, m, k))
        t_all, a_all, r_all = t_all + t, a_all + a, r_all + sum(1 for x in ms[m:k] if x[2] == W.RDONE)
        if k < len(ms):
            return (BATCH if ms[k][3] > e else STALE), (b, k), E, taken, t_all, a_all, r_all
        b, m = b + 1, 0


def repack(mbufs, taken):
    """the taken messages alone, each mbuf's share an mbuf of its own (same src)"""
    out = []
    for b, m, k in taken:
        ms = parse_mbuf(mbufs[b])
        src = struct.unpack_from("<I", mbufs[b], 4)[0]
        out.append(mbuf([mbufs[b][o:o + sz] for o, sz, *_ in ms[m:k]], src))
    return out


def stream(mbufs):
    return C0.stream(mbufs)


def host_cfg(max_req=0, **kw):
    d = dict(node_id=NODE, node_cnt=NODE_CNT, part_cnt=PART_CNT, synth_table_size=ROWS, max_req=max_req, calvin=True)
    d.update(kw)
    return d


def host_decode(mbufs, max_req=0, **kw):
    """mbufs of one batch id through the host decoder with ample capacity: one epoch (WireEpoch)"""
    w = WireIngress(L.YCSB, 1 << 16, 1 << 20, **host_cfg(max_req, **kw))
    if mbufs:
        buf, off = stream(mbufs)
        assert w.feed_buffer(buf, off) == []
    return w.take()


def host_stop(mbufs, cur=(0, 0), E=None):
    """dv_wire_decode_batches from the cursor with ample capacity: (stop,
    cursor, txns, accesses, rdones, batch id); the first mbuf trimmed to its
    messages from the cursor (the host cursor cannot skip)"""
    b0, m0 = cur
    first = []
    if b0 < len(mbufs):
        ms = parse_mbuf(mbufs[b0])
        first = [mbuf([mbufs[b0][o:o + sz] for o, sz, *_ in ms[m0:]], struct.unpack_from("<I", mbufs[b0], 4)[0])]
    rest = first + list(mbufs[b0 + 1:])
    w = WireIngress(L.YCSB, 1 << 16, 1 << 20, **host_cfg())
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
def good_cases(seed=7, bid=9):
    """[(name, mbuf bytes, txns, accesses, rdones)], all of batch `bid`: every
    message shape the issue names, garbage in the padding and latency fields"""
    rng = np.random.default_rng(seed)
    out, msgs, lens, k = [], [], [], 0
    for n in (0, 1, 10, 128):
        for p in (0, 1, 4):
            msgs.append(message(_reqs(rng, n), list(range(p)), bid, 1000 + k, 3 * k + 1, rng))
            lens.append(n)
            k += 1
    pos = 0
    for b in W.batches(NODE, 5, msgs):
        cnt = struct.unpack_from("<I", b, 8)[0]
        out.append((f"shapes{pos}", b, cnt, sum(lens[pos:pos + cnt]), 0))
        pos += cnt
    out.append(("one_rdone", mbuf([rdone(bid, rng)], 6), 0, 0, 1))
    b48 = mbuf([rdone(bid, rng) for _ in range(48)], 7)
    assert len(b48) == 4044
    out.append(("rdones_48", b48, 0, 0, 48))
    # exactly 4,096 bytes: 12 + (108 + 8 + 24 * 128) + (108 + 8 + 24 * 28) + 108
    full = mbuf([message(_reqs(rng, 128), [3], bid, 300, 7, rng), message(_reqs(rng, 28), [2], bid, 301, 8, rng),
                 message([], [], bid, 302, 9, rng)], 8)
    assert len(full) == 4096
    out.append(("full_4096", full, 3, 156, 0))
    out.append(("query_then_rdone", mbuf([message(_reqs(rng, 10), [1], bid, 77, 5, rng), rdone(bid, rng)], 6), 1, 10, 1))
    # (what the YCSB entry's cases call malformed and CALVIN does not: an RDONE behind a query)
    out.append(("rtype_rdone", mbuf([message(_reqs(rng, 3), [0], bid, 9, 1, rng), rdone(bid)]), 1, 3, 1))
    # past lane 64 of the flat loops: 90 partitions in an mbuf, 128 requests in a message; an RDONE behind each
    p90 = [message([], [i % PART_CNT, 1, 2], bid, 400 + i, 50 + i, rng) for i in range(30)]
    assert len(mbuf(p90)) == 30 * 132 + 12 == 3972 and len(mbuf(p90 + [rdone(bid, rng)])) <= 4096
    out.append(("partitions_90", mbuf(p90 + [rdone(bid, rng)], 7), 30, 0, 1))
    out.append(("requests_128", mbuf([message(_reqs(rng, 128), [0], bid, 500, 90, rng), rdone(bid, rng)], 7), 1, 128, 1))
    return out


def malformed_cases(seed=11, bid=9):
    """[(name, mbuf bytes, max_req)]: every YCSB kind of
    test_wire_device_cases.malformed_cases re-encoded with batch ids
    (rtype_rdone is well-formed under CALVIN: good_cases), then CALVIN's own."""
    rng = np.random.default_rng(seed)
    ok = lambda n=3, p=(0,): message(_reqs(rng, n), list(p), bid, 9, 4, rng)  # noqa: E731
    q = lambda reqs, parts, **kw: message(reqs, parts, bid, 1, 6, rng, **kw)  # noqa: E731
    m = []
    m.append(("len_below_12", struct.pack("<II", NODE, 5), 0))
    m.append(("len_above_4096", mbuf([ok(128), ok(40)]) + b"\0" * 100, 0))
    assert len(m[-1][1]) > 4096
    m.append(("dest_not_this_node", mbuf([ok()], dest=NODE + 1), 0))
    m.append(("src_is_this_node", mbuf([ok()], src=NODE), 0))
    m.append(("count_zero", mbuf([], count=0), 0))
    m.append(("count_zero_with_bytes", mbuf([ok()], count=0), 0))
    m.append(("count_one_more", mbuf([ok(), ok()], count=3), 0))
    m.append(("count_one_less", mbuf([ok(), ok()], count=1), 0))
    m.append(("count_huge", mbuf([ok()], count=0xFFFFFFFF), 0))
    m.append(("trailing_bytes", mbuf([ok()]) + b"\0" * 8, 0))
    m.append(("truncated_header", mbuf([ok()])[:12 + 60], 0))
    m.append(("rtype_cl_rsp", mbuf([ok(), q(_reqs(rng, 2), [0], rtype=W.CL_RSP)]), 0))
    m.append(("rdone_shaped_like_a_query", mbuf([q(_reqs(rng, 2), [0], rtype=W.RDONE)]), 0))
    m.append(("partitions_65", mbuf([q(_reqs(rng, 1), [0] * 65)]), 0))
    m.append(("partition_out_of_range", mbuf([ok(), q(_reqs(rng, 4), [0, PART_CNT])]), 0))
    m.append(("requests_129", mbuf([q(_reqs(rng, 129), [0])]), 0))
    m.append(("requests_above_max_req", mbuf([q(_reqs(rng, 17), [0])]), 16))
    m.append(("requests_past_the_end", mbuf([ok(), q(_reqs(rng, 4), [0], n_reqs=5)]), 0))
    m.append(("partitions_past_the_end", mbuf([q([], [0, 1], n_parts=40)]), 0))
    m.append(("acctype_2", mbuf([q([(0, 1), (2, 2), (1, 3)], [0])]), 0))
    m.append(("acctype_scan", mbuf([q([(3, 1)], [0])]), 0))
    m.append(("acctype_high_bits", mbuf([q([(1 << 8, 1)], [0])]), 0))
    m.append(("key_is_table_size", mbuf([ok(5), q([(0, ROWS)], [0])]), 0))
    m.append(("key_high_bits", mbuf([q([(1, 1 << 32)], [0])]), 0))
    m.append(("requests_wrap_2_61_plus_1", mbuf([q(_reqs(rng, 1), [0], n_reqs=(1 << 61) + 1)]), 0))
    m.append(("partitions_wrap_2_61", mbuf([q(_reqs(rng, 1), [], n_parts=1 << 61)]), 0))
    m.append(("requests_2_32_plus_1", mbuf([q(_reqs(rng, 1), [0], n_reqs=(1 << 32) + 1)]), 0))
    # the twins of good_cases' partitions_90 / requests_128: the bad field past flat index 63 of its loop
    parts = [[0, 1, 2] for _ in range(30)]
    parts[82 // 3][82 % 3] = PART_CNT
    m.append(("partition_82_of_90_out_of_range", mbuf([q([], p) for p in parts] + [rdone(bid, rng)]), 0))
    assert len(m[-1][1]) == 3972 + 84
    reqs = _reqs(rng, 128)
    reqs[100] = (reqs[100][0], ROWS)
    m.append(("request_100_of_128_key_is_table_size", mbuf([q(reqs, [0]), rdone(bid, rng)]), 0))
    # CALVIN's own
    m.append(("batch_id_max_on_a_query", mbuf([ok(), message(_reqs(rng, 2), [0], U64, 1, 6, rng)]), 0))
    m.append(("batch_id_max_on_an_rdone", mbuf([ok(), rdone(U64, rng)]), 0))
    m.append(("rdone_with_trailing_bytes", mbuf([ok(), rdone(bid, rng) + b"\0" * 8]), 0))
    m.append(("unknown_rtype", mbuf([ok(), header(7, 1, bid, rng)]), 0))
    m.append(("forty_nine_rdones", mbuf([rdone(bid, rng) for _ in range(49)]), 0))
    m.append(("bad_mbuf_of_the_next_batch", mbuf([message([(2, 1)], [0], bid + 1, 1, 6, rng)]), 0))
    return m


OFF_CASES = C0.OFF_CASES


def cut_cases(seed=13, e=9):
    """[(name, mbufs, cursor, E or None)]: streams that stop at a batch
    boundary or a stale message, or run to their end"""
    rng = np.random.default_rng(seed)
    tid = iter(range(100, 10_000))
    q = lambda bid, n=2: message(_reqs(rng, n), [0], bid, 500 + n, next(tid), rng)  # noqa: E731
    head = [mbuf([q(e, 3), q(e, 0)], 5), mbuf([q(e, 1)], 6)]
    out = []
    out.append(("cut_at_message_1", head + [mbuf([rdone(e, rng), q(e + 1), q(e + 1)], 5), mbuf([q(e + 1)], 5)],
                (0, 0), None))
    out.append(("cut_at_a_middle_message",
                head + [mbuf([q(e), q(e, 5), rdone(e, rng), q(e + 1), q(e + 1, 4), rdone(e + 1, rng)], 5)], (0, 0), e))
    out.append(("cut_at_the_last_message", head + [mbuf([q(e), q(e), rdone(e, rng), q(e + 2)], 5)], (0, 0), None))
    out.append(("mbuf_wholly_of_the_later_batch", head + [mbuf([q(e + 1), rdone(e + 1, rng)], 5)], (0, 0), None))
    out.append(("first_message_already_later", [mbuf([q(e + 1), q(e + 1)], 5)] + head, (0, 0), e))
    out.append(("E_from_a_cursor_inside_an_mbuf",
                [mbuf([q(e - 1), rdone(e - 1, rng), q(e), q(e, 4)], 5), mbuf([q(e), rdone(e, rng), q(e + 1)], 6)],
                (0, 2), None))
    out.append(("cursor_at_the_last_message", [mbuf([q(e - 1), q(e)], 5), mbuf([rdone(e, rng)], 5)], (0, 1), None))
    out.append(("runs_to_the_end", head + [mbuf([q(e), rdone(e, rng)], 5)], (0, 0), e))
    out.append(("nothing_left", head, (2, 0), e))
    out.append(("stale_at_an_mbufs_first_message", head + [mbuf([q(e - 1), q(e)], 5)], (0, 0), None))
    out.append(("stale_mid_mbuf", head + [mbuf([q(e), q(e, 4), q(e - 3), q(e)], 5)], (0, 0), e))
    out.append(("stale_at_the_cursor", [mbuf([q(e - 1), q(e)], 5)], (0, 0), e))
    return out


# ---- on the host decoder alone
def _open(b, max_req=0):
    cfg = L.WireCfg(L.YCSB, 1, NODE, NODE_CNT, PART_CNT, max_req, ROWS, None)
    buf = np.frombuffer(b, np.uint8)
    cur = L.WireCursor()
    return L.lib().dv_wire_open(ctypes.byref(cfg), buf.ctypes.data_as(ctypes.c_void_p), len(buf), ctypes.byref(cur))


def test_good_cases_are_accepted_with_the_expected_counts():
    cases = good_cases()
    assert {c[0] for c in cases} >= {"one_rdone", "rdones_48", "full_4096"} and len(cases) >= 8
    lens = set()
    for name, b, txns, accs, rd in cases:
        assert _open(b) == L.DV_OK, name
        ep = host_decode([b])
        assert (ep.n_txn, ep.n_acc, ep.rdone, ep.batch_id) == (txns, accs, rd, 9), name
        ms = parse_mbuf(b)
        assert (sum(1 for x in ms if x[2] == W.CL_QRY), sum(x[4] for x in ms)) == (txns, accs), name
        lens |= set(np.diff(ep.txn_begin.astype(np.int64)).tolist())
    assert lens >= {0, 1, 10, 128}
    assert max(len(c[1]) for c in cases) == 4096


@pytest.mark.parametrize("case", malformed_cases(), ids=lambda c: c[0])
def test_malformed_cases_are_refused_by_the_host_decoder(case):
    name, b, max_req = case
    assert _open(b, max_req) == L.DV_ERR_ARG
    if max_req:  # (it is the limit that refuses it)
        assert _open(b, 0) == L.DV_OK


def test_every_ycsb_malformed_kind_is_re_encoded():
    mine = {c[0] for c in malformed_cases()}
    assert {c[0] for c in C0.malformed_cases()} - mine == {"rtype_rdone"}
    assert "rtype_rdone" in {c[0] for c in good_cases()}


@pytest.mark.parametrize("case", cut_cases(), ids=lambda c: c[0])
def test_the_model_stops_where_the_host_decoder_stops(case):
    name, mbufs, cur, E = case
    for b in mbufs:
        assert _open(b) == L.DV_OK
    stop, at, e_out, taken, t, a, r = model(mbufs, set(), cur, E)
    h_stop, h_at, h_t, h_a, h_r, h_e = host_stop(mbufs, cur, E)
    assert (stop, at, t, a, r) == (h_stop, h_at, h_t, h_a, h_r)
    assert e_out == h_e or (not taken and h_e == E)
    # ... and the taken messages alone decode to the same epoch
    ref = host_decode(repack(mbufs, taken))
    assert (ref.n_txn, ref.n_acc, ref.rdone) == (t, a, r)
    if taken:
        assert ref.batch_id == e_out
    # resuming at the cursor reproduces the host decoder's next epoch
    if stop == BATCH:
        stop2, at2, e2, taken2, t2, a2, r2 = model(mbufs, set(), at, None)
        h2 = host_stop(mbufs, at, None)
        assert (stop2, at2, t2, a2, r2, e2) == h2
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


# ---- the C ABI without a device
def _out(**kw):
    one = 0x1000  # (never dereferenced: every call here is refused before a launch)
    d = dict(max_txn=16, pad_=0, max_acc=160, txn_begin=one, n_acc_dev=None, recs32=None, keys=one, types=one,
             acc_txn=one, owner=None, txn_id=None, client_startts=None, return_node=None)
    d.update(kw)
    return L.WireDevOut(**d)


def _pos(**kw):
    d = dict(batch=0, msg=0, n_txn=0, rdone=0, n_acc=0, batch_id=U64, max_txn_acc=0, stop=77)
    d.update(kw)
    return L.WireCalvinPos(**d)


def good_cfg(**kw):
    return L.WireCfg(**{**dict(workload=L.YCSB, calvin=1, node_id=NODE, node_cnt=NODE_CNT, part_cnt=PART_CNT,
                               max_req=0, synth_table_size=ROWS, tpcc=None), **kw})


def ingest(ctx, cfg, out, pos, buf=0x1000, off=0x1000, n_batches=3):
    return L.lib().dv_wire_ingest_device_calvin(ctx, ctypes.byref(cfg) if cfg is not None else None, buf, 64, off,
                                                n_batches, ctypes.byref(out) if out is not None else None,
                                                ctypes.byref(pos) if pos is not None else None)


def refused_arguments():
    """[(name, cfg, out, pos)]: argument sets dv_wire_ingest_device_calvin
    refuses before any launch, whatever the context (shared with the GPU
    test, which passes a live one); n_batches is 3"""
    return [
        ("not_calvin", good_cfg(calvin=0), _out(), _pos()),
        ("tpcc", good_cfg(workload=L.TPCC), _out(), _pos()),
        ("part_cnt_zero", good_cfg(part_cnt=0), _out(), _pos()),
        ("node_cnt_zero", good_cfg(node_cnt=0), _out(), _pos()),
        ("no_txn_begin", good_cfg(), _out(txn_begin=None), _pos()),
        ("no_keys", good_cfg(), _out(keys=None), _pos()),
        ("no_types", good_cfg(), _out(types=None), _pos()),
        ("no_acc_txn", good_cfg(), _out(acc_txn=None), _pos()),
        ("records_alone", good_cfg(), _out(keys=None, types=None, acc_txn=None, recs32=0x1000), _pos()),
        ("recs32_with_a_table_above_2_31", good_cfg(synth_table_size=(1 << 31) + 1), _out(recs32=0x1000), _pos()),
        ("max_txn_zero", good_cfg(), _out(max_txn=0), _pos()),
        ("max_txn_above_2_24", good_cfg(), _out(max_txn=(1 << 24) + 1), _pos()),
        ("max_acc_2_32", good_cfg(), _out(max_acc=1 << 32), _pos()),
        ("cursor_past_the_stream", good_cfg(), _out(), _pos(batch=4)),
        ("message_cursor_at_the_end", good_cfg(), _out(), _pos(batch=3, msg=1)),
        ("n_txn_above_max_txn", good_cfg(), _out(), _pos(n_txn=17)),
        ("n_acc_above_max_acc", good_cfg(), _out(), _pos(n_acc=161)),
    ]


def test_the_new_entry_rejects_null_and_unsupported_arguments():
    """DV_ERR_ARG before any device is touched, *pos as it was"""
    assert ingest(None, good_cfg(), _out(), _pos()) == L.DV_ERR_ARG
    assert ingest(None, None, None, None, 0, 0) == L.DV_ERR_ARG
    for name, c, o, p in refused_arguments():
        before = bytes(p)
        assert ingest(None, c, o, p) == L.DV_ERR_ARG, name
        assert bytes(p) == before, name


def test_the_existing_entries_still_refuse_calvin():
    cfg = good_cfg()
    r = L.WireDevResult()
    o = C0._out()
    assert L.lib().dv_wire_ingest_device(None, ctypes.byref(cfg), 0x1000, 64, 0x1000, 1, 0, ctypes.byref(o), 0,
                                         ctypes.byref(r)) == L.DV_ERR_ARG
    assert ("calvin" in {c[0] for c in C0.refused_arguments()})
    t = L.WireTpccDevOut()
    assert L.lib().dv_wire_ingest_device_tpcc(None, ctypes.byref(cfg), 0x1000, 64, 0x1000, 1, 0, ctypes.byref(t), 0,
                                              ctypes.byref(r)) == L.DV_ERR_ARG


def test_struct_layout_and_stop_codes_match_the_header(tmp_path):
    import os
    import subprocess
    cls, name = L.WireCalvinPos, "dv_wire_calvin_pos"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dvcc.h"', "int main(void) {",
             f'printf("{name} %zu\\n", sizeof({name}));']
    for f, _ in cls._fields_:
        lines.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    for s in ("END", "BATCH", "CAPACITY", "WINDOW", "MALFORMED", "STALE"):
        lines.append(f'printf("{s} %d\\n", DV_WIRE_STOP_{s});')
    lines.append("return 0; }")
    src = tmp_path / "sz.c"
    src.write_text("\n".join(lines))
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.check_call(["gcc", "-I", inc, str(src), "-o", str(tmp_path / "sz")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "sz")]).decode().splitlines())
    assert int(got[name]) == ctypes.sizeof(cls) == 40
    for f, _ in cls._fields_:
        assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, f
    assert [int(got[s]) for s in ("END", "BATCH", "CAPACITY", "WINDOW", "MALFORMED", "STALE")] == [
        L.WIRE_STOP_END, L.WIRE_STOP_BATCH, L.WIRE_STOP_CAPACITY, L.WIRE_STOP_WINDOW, L.WIRE_STOP_MALFORMED,
        L.WIRE_STOP_STALE] == [END, BATCH, CAPACITY, WINDOW, MALFORMED, STALE]
