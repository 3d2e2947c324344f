"""The CALVIN sequencer's host functions under a TPC-C cfg (dv_wire_sequence,
dv_wire_sequence_acks: csrc/wire.cpp) against the independent model of
tests/wire_seq_tpcc.py, a known answer packed by hand, dv_wire_open's verdict
on the same messages, and a sanitizer program of its own
(tests/cpp/wire_sequence_tpcc_test.cpp).  No GPU: the device entries are held
against these host functions in test_wire_sequence_tpcc_gpu.py."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import wire_fmt as W
import wire_seq as S
import wire_seq_tpcc as ST
from dvcc import _lib as L
from dvcc import tpcc as T
from dvcc import wire as DW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(t):
    return T.tpcc_params(t["num_wh"], t["dist"], t["cust"], t["items"], part_cnt=t["part_cnt"])


def host(mbufs, batch_id, k, first=0, **extra):
    buf, off = S.queue(mbufs)
    return DW.sequence_host(buf, off, batch_id, node_id=k["node_id"], node_cnt=k["node_cnt"], part_cnt=k["part_cnt"],
                            n_dest=k["n_dest"], max_txn=k["max_txn"], first_batch=first, params=params(k["tp"]),
                            **extra)


def agrees(b, m, k):
    """a SequencedBatch against the model's dict"""
    r = b.result
    assert (r.status, r.n_taken, r.n_txn, r.n_msgs) == (m["status"], m["n_taken"], m["n_txn"], m["n_msgs"])
    flat = [x for d in m["per_dest"] for x in d]
    assert r.n_out == len(flat) and r.n_bytes == sum(len(x) for x in flat)
    assert b.mbufs() == flat
    first = np.cumsum([0] + [len(d) for d in m["per_dest"]])
    assert b.dest_first.tolist() == first.tolist()
    for d in range(k["node_cnt"]):
        assert b.mbufs(d) == m["per_dest"][d]
    n = r.n_txn
    got = list(zip(b.wait_client[:n].tolist(), b.wait_startts[:n].tolist(), b.wait_acks[:n].tolist()))
    assert got == m["wait"]
    assert not b.out[r.n_bytes:].any() and not b.batch_off[r.n_out + 1:].any() and not b.wait_acks[n:].any()


def untouched(b):
    return not (b.out.any() or b.batch_off.any() or b.dest_first.any() or b.wait_client.any() or
                b.wait_startts.any() or b.wait_acks.any())


def test_known_answer_two_nodes_four_txns():
    """Sequencer 0 of two nodes, 4 warehouses over 2 partitions (warehouses 1
    and 3 on node 0, 2 and 4 on node 1), clients 2 and 3: a local Payment, a
    Payment whose customer is on the other node, a NewOrder with items on both
    nodes, and a Payment that carries three leftover items of the other
    node's warehouses, which name no participant -- every byte packed here."""
    E = 5

    def body(tt, w, d, c, d_w, c_w, c_d, h, items, ol_cnt, entry, flags=(False, False)):
        return (struct.pack("<7Q", tt, w, d, c, d_w, c_w, c_d) + bytes(16) + struct.pack("<QBQ", h, 0, len(items)) +
                b"".join(struct.pack("<QQQ", *i) for i in items) + struct.pack("<BBQQ", *flags, ol_cnt, entry))

    def client(cst, parts, b):  # a client's message: no txn id, no batch id, its own clocks
        return (struct.pack("<IQQQ", 3, W.U64_MAX, W.U64_MAX, 0x1122) + struct.pack("<7d", *(1.5,) * 7) +
                struct.pack("<QQ", cst, len(parts)) + b"".join(struct.pack("<Q", p) for p in parts) + b)

    def stamped(k, cst, parts, b):  # as the sequencer forwards it: txn_id 0 + 2 k, the clocks zeroed
        return (struct.pack("<IQQ", 3, 2 * k, E) + bytes(64) + struct.pack("<QQ", cst, len(parts)) +
                b"".join(struct.pack("<Q", p) for p in parts) + b)

    left = [(7, 2, 1), (8, 4, 1), (9, 2, 1)]
    txns = [(0xA1, [0], body(1, 1, 3, 7, 1, 3, 2, 500, [], 0, 0)),                  # Payment w 1, c_w 3: node 0
            (0xA2, [0, 1], body(1, 3, 3, 7, 3, 2, 2, 600, [], 0, 0)),               # Payment w 3, c_w 2: both
            (0xA3, [0, 1], body(2, 1, 4, 9, 0, 0, 0, 0, [(11, 1, 5), (12, 4, 6)], 2, 77, (True, True))),  # both
            (0xA4, [0], body(1, 1, 3, 7, 1, 1, 2, 700, left, 3, 0))]                # Payment w 1: node 0 alone
    sizes = [len(client(*t)) for t in txns]
    assert sizes == [215, 223, 223 + 48, 215 + 72] and all(s % 4 == 3 for s in sizes)
    mbufs = [struct.pack("<III", 0, 2, 2) + client(*txns[0]) + client(*txns[1]),
             struct.pack("<III", 0, 3, 2) + client(*txns[2]) + client(*txns[3])]
    t = ST.tp(num_wh=4, part_cnt=2)
    b = host(mbufs, E, ST.kw(node_id=0, node_cnt=2, part_cnt=2, tp_=t, n_dest=4))
    rdone = struct.pack("<IQQ", 19, W.U64_MAX, E) + bytes(64)
    want = [struct.pack("<III", 0, 0, 5) + b"".join(stamped(k, *txns[k]) for k in (0, 1, 2, 3)) + rdone,
            struct.pack("<III", 1, 0, 3) + b"".join(stamped(k, *txns[k]) for k in (1, 2)) + rdone]
    assert b.mbufs() == want
    assert b.dest_first.tolist() == [0, 1, 2]
    assert [len(x) for x in want] == [12 + sum(sizes) + 84, 12 + sizes[1] + sizes[2] + 84] == [1092, 590]
    assert b.batch_off[:3].tolist() == [0, 1092, 1682]  # (node 1's RDONE starts at byte 1,598: 2 mod 4)
    r = b.result
    assert (r.status, r.n_taken, r.n_txn, r.n_out, r.n_msgs, r.n_bytes) == (0, 2, 4, 2, 6, len(b"".join(want)))
    assert b.wait_client[:4].tolist() == [2, 2, 3, 3] and b.wait_startts[:4].tolist() == [0xA1, 0xA2, 0xA3, 0xA4]
    assert b.wait_acks[:4].tolist() == [1, 2, 2, 1]
    # the model reads the same bytes the same way
    agrees(b, ST.sequence(mbufs, E, **ST.kw(node_id=0, node_cnt=2, part_cnt=2, tp_=t, n_dest=4)),
           dict(node_cnt=2))


CASES = ST.sequence_cases()


@pytest.mark.parametrize("name,mbufs,batch_id,k", CASES, ids=[c[0] for c in CASES])
def test_sequence_against_the_model(name, mbufs, batch_id, k):
    m = ST.sequence(mbufs, batch_id, **k)
    assert m["status"] == ST.OK and m["n_taken"] == len(mbufs)
    agrees(host(mbufs, batch_id, k), m, k)
    if name == "idle_dest":
        assert [len(d) for d in m["per_dest"]] == [1, 1, 1] and m["per_dest"][1] == W.batches(1, 0, [W.rdone(batch_id)])
    if name == "nodes64":
        # (warehouse 65 is partition 64, node 0, as 101 would be; 102 is partition 1, node 1)
        assert m["wait"][0][2] == 63 and m["wait"][1][2] == 2 and m["n_msgs"] > 100


FILLS = ST.fill_cases()


@pytest.mark.parametrize("name,mbufs,batch_id,k,n_out,last", FILLS, ids=[c[0] for c in FILLS])
def test_an_mbuf_filled_to_the_byte_and_eight_bytes_over(name, mbufs, batch_id, k, n_out, last):
    m = ST.sequence(mbufs, batch_id, **k)
    b = host(mbufs, batch_id, k)
    agrees(b, m, k)
    got = b.mbufs()
    assert len(got) == n_out and len(got[-1]) == last
    if name.startswith("msgs_fill") or name.startswith("rdone_fills"):
        assert len(got[0]) == 4096
    else:
        assert len(got[0]) < 4096


@pytest.mark.parametrize("size", [215, 1703])
@pytest.mark.parametrize("n_msgs", [254, 255, 256, 257, 511, 513, 528])
def test_lists_at_the_device_cut_searchs_tile_against_the_model(n_msgs, size):
    """the host function at the list lengths the GPU suite holds the device against it"""
    k = ST.kw(max_txn=768, tp_=ST.tp(num_wh=4))
    mbufs = ST.sized_queue(n_msgs, size)
    agrees(host(mbufs, 31, k), ST.sequence(mbufs, 31, **k), k)


def test_max_txn_exact_and_one_below():
    _, mbufs, e, k = next(c for c in CASES if c[0] == "two_nodes")
    n = ST.sequence(mbufs, e, **k)["n_txn"]
    for max_txn in (n, n - 1, 1):
        kk = dict(k, max_txn=max_txn)
        m = ST.sequence(mbufs, e, **kk)
        assert m["status"] == (ST.OK if max_txn == n else ST.MORE if max_txn == n - 1 else ST.ERR)
        agrees(host(mbufs, e, kk), m, kk)
    kk = dict(k, max_txn=n - 1)
    first = ST.sequence(mbufs, e, **kk)["n_taken"]
    m = ST.sequence(mbufs, e + 1, first=first, **kk)
    assert m["status"] == ST.OK and 0 < m["n_txn"] < n
    agrees(host(mbufs, e + 1, kk, first=first), m, kk)


def test_cap_and_max_batches_exact_and_one_below():
    _, mbufs, e, k = next(c for c in CASES if c[0] == "mixed_cuts")
    m = ST.sequence(mbufs, e, **k)
    free = host(mbufs, e, k).result
    agrees(host(mbufs, e, k, cap=free.n_bytes, max_batches=free.n_out), m, k)
    for extra in (dict(cap=free.n_bytes - 1), dict(max_batches=free.n_out - 1)):
        b = host(mbufs, e, k, **extra)
        r = b.result
        assert r.status == L.DV_ERR_ARG and (r.n_bytes, r.n_out, r.n_txn, r.n_taken) == (
            free.n_bytes, free.n_out, free.n_txn, free.n_taken)
        assert untouched(b)


MALFORMED = ST.malformed_cases()


@pytest.mark.parametrize("name,mbufs,k,n_taken,stamped", MALFORMED, ids=[c[0] for c in MALFORMED])
def test_a_malformed_mbuf_stops_the_batch_and_dv_wire_open_refuses_it_too(name, mbufs, k, n_taken, stamped):
    m = ST.sequence(mbufs, 4, **k)
    accepted = name == "payment_items_unchecked"
    assert m["status"] == (ST.OK if accepted else ST.ERR) and m["n_taken"] == n_taken
    agrees(host(mbufs, 4, k), m, k)
    if stamped is None:
        return
    # one rule, not two: the same messages with a batch id, addressed to a CALVIN TPC-C node from another
    pp = params(k["tp"])
    cfg = L.WireCfg(L.TPCC, 1, 0, 2, k["part_cnt"], 0, 0, ctypes.pointer(pp))
    b = np.frombuffer(struct.pack("<II", 0, 1) + stamped[8:] if len(stamped) >= 12 else stamped, np.uint8).copy()
    rc = L.lib().dv_wire_open(ctypes.byref(cfg), b.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(b),
                              ctypes.byref(L.WireCursor()))
    assert rc == (L.DV_OK if accepted else L.DV_ERR_ARG)


def test_a_tpcc_cfg_needs_its_params():
    mbufs, k = [W.batches(0, 2, [ST.payment(1)])[0]], ST.kw()
    assert host(mbufs, 4, k).result.status == L.DV_OK
    buf, off = S.queue(mbufs)
    b = host(mbufs, 4, k)
    sin = L.WireSeqIn(buf.ctypes.data, len(buf), off.ctypes.data, 1, 0, 4, 3, 8)
    sout = L.WireSeqOut(b.out.ctypes.data, len(b.out), b.batch_off.ctypes.data, 2, 0, b.dest_first.ctypes.data,
                        b.wait_client.ctypes.data, b.wait_startts.ctypes.data, b.wait_acks.ctypes.data)
    before = b.out.copy()
    for cfg in (L.WireCfg(L.TPCC, 1, 0, 1, 1, 0, 0, None),
                L.WireCfg(L.TPCC, 1, 0, 1, 1, 0, 0, ctypes.pointer(T.tpcc_params(4, part_cnt=5)))):  # (knobs refused)
        res = L.WireSeqResult(status=7)
        assert L.lib().dv_wire_sequence(cfg, sin, sout, res) == L.DV_ERR_ARG and res.status == 7
        assert (b.out == before).all()
    pp = params(k["tp"])
    res = L.WireSeqResult(status=7)
    assert L.lib().dv_wire_sequence(L.WireCfg(L.TPCC, 1, 0, 1, 1, 0, 0, ctypes.pointer(pp)), sin, sout, res) == L.DV_OK


# ---- the acks in: the workload changes nothing
def _acks(wait, batch_id, calls, k, pp):
    wc = np.array([w[0] for w in wait], np.uint32)
    ws = np.array([w[1] for w in wait], np.uint64)
    wa = np.array([w[2] for w in wait], np.uint32)
    outs = []
    for mbufs in calls:
        buf, off = S.queue(mbufs)
        out, boff, res = DW.sequence_acks_host(buf, off, batch_id, wc, ws, wa, params=pp, **k)
        outs.append((out.tobytes(), boff.tolist(), [getattr(res, f) for f, _ in res._fields_], wa.tolist()))
    return outs


ACKS = S.ack_cases()


@pytest.mark.parametrize("name,wait,batch_id,calls,k", ACKS, ids=[c[0] for c in ACKS])
def test_acks_under_a_tpcc_cfg_equal_the_ycsb_run(name, wait, batch_id, calls, k):
    ycsb = _acks(wait, batch_id, calls, k, None)
    assert _acks(wait, batch_id, calls, k, T.tpcc_params(4, part_cnt=2)) == ycsb
    assert any(o[2][0] == L.DV_OK for o in ycsb) or name not in ("all_in_one", "node_per_call")
    # and a TPC-C cfg without params is refused before the acks are read
    wa = np.array([w[2] for w in wait], np.uint32)
    res = L.WireSeqAckResult(status=7)
    cfg = L.WireCfg(L.TPCC, 1, k["node_id"], k["node_cnt"], 1, 0, 0, None)
    assert L.lib().dv_wire_sequence_acks(cfg, L.WireSeqAckIn(), L.WireRspOut(), res) == L.DV_ERR_ARG and res.status == 7
    assert wa.tolist() == [w[2] for w in wait]


def test_sanitizer_program(tmp_path):
    """tests/cpp/wire_sequence_tpcc_test.cpp: every prefix of a valid TPC-C
    client mbuf (a Payment and a 62-item NewOrder) refused without a read out
    of bounds -- built with the address and undefined-behaviour sanitizers,
    run as a child process."""
    exe = str(tmp_path / "wire_sequence_tpcc_test")
    csrc = os.path.join(ROOT, "deneva-plus_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cpp", "wire_sequence_tpcc_test.cpp"),
                           os.path.join(csrc, "wire.cpp"), os.path.join(csrc, "tpcc_gen.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), r.stdout + r.stderr
