"""The CALVIN sequencer's host functions (dv_wire_sequence,
dv_wire_sequence_acks: csrc/wire.cpp) against the independent model of
tests/wire_seq.py, a hand-written known answer, and a sanitizer program of its
own (tests/cpp/wire_sequence_test.cpp).  No GPU: the device entries are held
against these host functions in test_wire_sequence_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

import wire_fmt as W
import wire_seq as S
from dvcc import _lib as L
from dvcc import wire as DW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(mbufs, batch_id, k, first=0, **extra):
    buf, off = S.queue(mbufs)
    return DW.sequence_host(buf, off, batch_id, node_id=k["node_id"], node_cnt=k["node_cnt"], part_cnt=k["part_cnt"],
                            synth_table_size=k["table"], n_dest=k["n_dest"], max_txn=k["max_txn"],
                            max_req=k["max_req"], first_batch=first, **extra)


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


def test_known_answer_two_nodes_three_txns():
    """Sequencer 1 of two nodes, part_cnt 2, clients 2 and 3: a txn on node 0
    alone, one on node 1 alone, one on both -- the bytes written out by hand."""
    q = lambda reqs, parts, cst: S.client_query(reqs, parts, cst, mq_time=0x1122, lat=(1.5,) * 7)  # noqa: E731
    mbufs = [W.batches(1, 2, [q([(0, 4)], [0], 0xA1), q([(1, 7)], [1], 0xA2)])[0],
             W.batches(1, 3, [q([(0, 2), (1, 9)], [0, 1], 0xA3)])[0]]
    b = host(mbufs, 5, S.kw(node_id=1, node_cnt=2, part_cnt=2, table=16, n_dest=4))
    hdr = lambda t, tid: f"{t:02x}000000" + f"{tid:02x}" + "00" * 7 + "05" + "00" * 7 + "00" * 64  # noqa: E731
    body = lambda cst, parts, reqs: (  # noqa: E731
        f"{cst:02x}" + "00" * 7 + f"{len(parts):02x}" + "00" * 7 + "".join(f"{p:02x}" + "00" * 7 for p in parts) +
        f"{len(reqs):02x}" + "00" * 7 +
        "".join(f"{a:02x}000000" + "00" * 4 + f"{k:02x}" + "00" * 7 + "5a" + "00" * 7 for a, k in reqs))
    rdone = "13000000" + "ff" * 8 + "05" + "00" * 7 + "00" * 64
    t0 = hdr(3, 1) + body(0xA1, [0], [(0, 4)])           # txn 0: id 1 + 2 * 0, node 0
    t1 = hdr(3, 3) + body(0xA2, [1], [(1, 7)])           # txn 1: id 3, node 1
    t2 = hdr(3, 5) + body(0xA3, [0, 1], [(0, 2), (1, 9)])  # txn 2: id 5, both
    want = ["00000000" "01000000" "03000000" + t0 + t2 + rdone, "01000000" "01000000" "03000000" + t1 + t2 + rdone]
    assert [m.hex() for m in b.mbufs()] == want
    assert b.dest_first.tolist() == [0, 1, 2] and b.batch_off[:3].tolist() == [0, len(want[0]) // 2, len("".join(want)) // 2]
    r = b.result
    assert (r.status, r.n_taken, r.n_txn, r.n_out, r.n_msgs, r.n_bytes) == (0, 2, 3, 2, 4, len("".join(want)) // 2)
    assert b.wait_client[:3].tolist() == [2, 2, 3] and b.wait_startts[:3].tolist() == [0xA1, 0xA2, 0xA3]
    assert b.wait_acks[:3].tolist() == [1, 1, 2]


CASES = S.sequence_cases()


@pytest.mark.parametrize("name,mbufs,batch_id,k", CASES, ids=[c[0] for c in CASES])
def test_sequence_against_the_model(name, mbufs, batch_id, k):
    m = S.sequence(mbufs, batch_id, **k)
    assert m["status"] == S.OK and m["n_taken"] == len(mbufs)
    agrees(host(mbufs, batch_id, k), m, k)


@pytest.mark.parametrize("size", [260, 244])
@pytest.mark.parametrize("n_msgs", [254, 255, 256, 257, 511, 512, 528])
def test_lists_at_the_device_cut_searchs_tile_against_the_model(n_msgs, size):
    """the host function at the list lengths the GPU suite holds the device against it"""
    k = S.kw(part_cnt=2, max_txn=768)
    mbufs = S.sized_queue(n_msgs, size)
    agrees(host(mbufs, 31, k), S.sequence(mbufs, 31, **k), k)


def test_the_rdone_fills_or_opens_an_mbuf():
    by = {c[0]: c for c in CASES}
    _, mbufs, e, k = by["rdone_fills"]
    b = host(mbufs, e, k)
    assert b.result.n_out == 1 and b.result.n_bytes == 4096
    for name in ("rdone_alone", "rdone_alone_29"):
        _, mbufs, e, k = by[name]
        b = host(mbufs, e, k)
        assert b.result.n_out == 2 and len(b.mbufs()[1]) == 12 + 84, name


def test_max_txn_exact_and_one_below():
    _, mbufs, e, k = next(c for c in CASES if c[0] == "two_nodes")
    n = S.sequence(mbufs, e, **k)["n_txn"]
    for max_txn in (n, n - 1, 1):
        kk = dict(k, max_txn=max_txn)
        m = S.sequence(mbufs, e, **kk)
        assert m["status"] == (S.OK if max_txn == n else S.MORE if max_txn == n - 1 else S.ERR)
        agrees(host(mbufs, e, kk), m, kk)
    # the rest of the queue as the next batch
    kk = dict(k, max_txn=n - 1)
    first = S.sequence(mbufs, e, **kk)["n_taken"]
    m = S.sequence(mbufs, e + 1, first=first, **kk)
    assert m["status"] == S.OK and 0 < m["n_txn"] < n
    agrees(host(mbufs, e + 1, kk, first=first), m, kk)


def test_cap_and_max_batches_exact_and_one_below():
    _, mbufs, e, k = next(c for c in CASES if c[0] == "mixed_cuts")
    m = S.sequence(mbufs, e, **k)
    free = host(mbufs, e, k).result
    agrees(host(mbufs, e, k, cap=free.n_bytes, max_batches=free.n_out), m, k)
    for extra in (dict(cap=free.n_bytes - 1), dict(max_batches=free.n_out - 1)):
        b = host(mbufs, e, k, **extra)
        r = b.result
        assert r.status == L.DV_ERR_ARG and (r.n_bytes, r.n_out, r.n_txn, r.n_taken) == (
            free.n_bytes, free.n_out, free.n_txn, free.n_taken)
        assert untouched(b)


MALFORMED = S.malformed_cases()


@pytest.mark.parametrize("name,mbufs,k,n_taken", MALFORMED, ids=[c[0] for c in MALFORMED])
def test_a_malformed_mbuf_stops_the_batch(name, mbufs, k, n_taken):
    m = S.sequence(mbufs, 4, **k)
    assert m["status"] == S.ERR and m["n_taken"] == n_taken
    agrees(host(mbufs, 4, k), m, k)


def test_calls_refused_before_the_bytes_are_read():
    mbufs, k = [W.batches(0, 2, [S.txn([1], 1)])[0]], S.kw()
    for change in (dict(node_cnt=65), dict(node_id=1), dict(part_cnt=0), dict(n_dest=0), dict(n_dest=257),
                   dict(max_txn=0)):
        with pytest.raises(L.DvccError):
            host(mbufs, 4, dict(k, **change))
    with pytest.raises(L.DvccError):
        host(mbufs, W.U64_MAX, k)
    with pytest.raises(L.DvccError):
        host(mbufs, 4, k, first=2)
    cfg = L.WireCfg(L.TPCC, 1, 0, 1, 1, 0, 100, None)
    res = L.WireSeqResult(status=7)
    assert L.lib().dv_wire_sequence(cfg, L.WireSeqIn(), L.WireSeqOut(), res) == L.DV_ERR_ARG and res.status == 7


# ---- the acks in
def run_acks(wait, batch_id, calls, k):
    """the host function and the model side by side, call after call"""
    wc = np.array([w[0] for w in wait], np.uint32)
    ws = np.array([w[1] for w in wait], np.uint64)
    wa = np.array([w[2] for w in wait], np.uint32)
    mw = list(wait)
    outs = []
    for mbufs in calls:
        buf, off = S.queue(mbufs)
        before = wa.copy()
        out, boff, res = DW.sequence_acks_host(buf, off, batch_id, wc, ws, wa, **k)
        m = S.acks(mbufs, batch_id, mw, **k)
        assert (res.status, res.first_bad, res.n_acks, res.n_skipped, res.n_done) == (
            m["status"], m["first_bad"], m["n_acks"], m["n_skipped"], len(m["done"]))
        got = [out[int(boff[j]):int(boff[j + 1])].tobytes() for j in range(res.n_batches)]
        assert got == m["replies"] and res.n_bytes == sum(len(x) for x in got)
        if m["status"] != S.OK:
            assert (wa == before).all() and not out.any() and not boff.any()
        mw = m["wait"]
        assert wa.tolist() == [w[2] for w in mw]
        outs.append((m, got))
    return outs, wa


ACKS = S.ack_cases()


@pytest.mark.parametrize("name,wait,batch_id,calls,k", ACKS, ids=[c[0] for c in ACKS])
def test_acks_against_the_model(name, wait, batch_id, calls, k):
    outs, wa = run_acks(wait, batch_id, calls, k)
    refused = {"over_ack", "foreign_txn", "txn_at_n_txn", "mbuf_47", "src_client", "dest_other", "no_batch_id",
               "not_an_ack", "length", "client_at_n_dest"}
    assert all((m["status"] == S.ERR) == (name in refused) for m, _ in outs)
    if name in ("all_in_one", "node_per_call", "reversed_nodes", "mbuf_45_46"):
        assert not wa.any()
        answered = sorted(t for _, got in outs for b in got for t, _, _ in S.parse_rsp_mbuf(b)[2])
        assert answered == [k["node_id"] + k["node_cnt"] * t for t in range(len(wait))]
        for _, got in outs:
            for b in got:
                dest, src, msgs = S.parse_rsp_mbuf(b)
                assert src == k["node_id"]
                for tid, bid, cst in msgs:
                    t = tid // k["node_cnt"]
                    assert bid == W.U64_MAX and (dest, cst) == wait[t][:2]


def test_the_order_of_the_acks_is_the_order_of_the_answers():
    """two txns of one client, two acks each: the txn whose last ack comes first is answered first"""
    k = dict(node_id=0, node_cnt=2, n_dest=3)
    wait = [(2, 10, 2), (2, 11, 2)]
    a = lambda t, src: S.ack_mbuf(0, src, [(2 * t, 6)])  # noqa: E731
    for calls, order in (([[a(0, 0), a(1, 0), a(1, 1), a(0, 1)]], [1, 0]), ([[a(0, 0), a(1, 0), a(0, 1), a(1, 1)]], [0, 1])):
        outs, _ = run_acks(wait, 6, calls, k)
        assert outs[0][0]["done"] == order
        assert [t // 2 for t, _, _ in S.parse_rsp_mbuf(outs[0][1][0])[2]] == order


def test_reply_capacities_are_decided_before_anything_changes():
    k = dict(node_id=0, node_cnt=1, n_dest=3)
    wc, ws, wa = np.array([1, 2, 1], np.uint32), np.array([7, 8, 9], np.uint64), np.array([1, 1, 1], np.uint32)
    buf, off = S.queue([S.ack_mbuf(0, 0, [(0, 3), (1, 3), (2, 3)])])
    for extra in (dict(cap=2 * 12 + 3 * 92 - 1), dict(max_batches=1)):
        out, boff, res = DW.sequence_acks_host(buf, off, 3, wc, ws, wa, **k, **extra)
        assert res.status == L.DV_ERR_ARG and (res.n_done, res.n_batches, res.n_bytes) == (3, 2, 2 * 12 + 3 * 92)
        assert wa.tolist() == [1, 1, 1] and not out.any() and not boff.any()
    out, boff, res = DW.sequence_acks_host(buf, off, 3, wc, ws, wa, **k, cap=2 * 12 + 3 * 92, max_batches=2)
    assert res.status == L.DV_OK and not wa.any()


def test_sanitizer_program(tmp_path):
    """tests/cpp/wire_sequence_test.cpp: every prefix of a valid client mbuf and
    of a valid ack mbuf refused without a read out of bounds, and the
    sequencer's workspace fields aligned, disjoint and inside the reported
    size -- built with the address and undefined-behaviour sanitizers, run as
    a child process."""
    exe = str(tmp_path / "wire_sequence_test")
    csrc = os.path.join(ROOT, "deneva-plus_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(ROOT, "tests", "cpp", "wire_sequence_test.cpp"), os.path.join(csrc, "wire.cpp"),
                           os.path.join(csrc, "tpcc_gen.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), r.stdout + r.stderr
