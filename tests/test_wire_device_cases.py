"""The cases of the device wire ingress (dv_wire_ingest_device), checked here on
the HOST decoder alone: every batch the GPU tests (tests/test_wire_device.py)
call good is accepted by dv_wire_open, every one they call malformed is
refused by it, and the txn / access counts they expect per batch are what
WireIngress decodes.  So the GPU tests never compare the device path against
a case its reference would not handle as assumed.  Also the C ABI's argument
checks that need no device.

Layout of a batch and its messages: tests/wire_fmt.py.  A YCSB CL_QRY of p
partitions and n requests is 100 + 8 p + 24 n bytes (header 76, client_startts
8, the two counts 8 each), so a 4,096-byte batch holds at most 40 messages.
"""
import ctypes
import struct

import numpy as np
import pytest

import wire_fmt as W
from dvcc import _lib as L
from dvcc.wire import WireIngress

NODE, NODE_CNT, PART_CNT, ROWS = 2, 3, 4, 1 << 16
U64 = (1 << 64) - 1


def message(reqs, parts, cst=0, rng=None, rtype=W.CL_QRY, n_parts=None, n_reqs=None):
    """One CL_QRY: reqs [(acctype, key)], parts [partition]; the requests'
    padding and value bytes random when rng is given (the decoders ignore
    them); n_parts / n_reqs: the counts written, when they are to lie."""
    body = b""
    for a, k in reqs:
        junk = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) if rng is not None else b"\x5a" * 12
        body += struct.pack("<I", a) + junk[:4] + struct.pack("<Q", k) + junk[4:]
    return (W.header(rtype) + struct.pack("<QQ", cst, len(parts) if n_parts is None else n_parts)
            + b"".join(struct.pack("<Q", p) for p in parts)
            + struct.pack("<Q", len(reqs) if n_reqs is None else n_reqs) + body)


def batch(msgs, src=5, dest=NODE, count=None):
    return struct.pack("<III", dest, src, len(msgs) if count is None else count) + b"".join(msgs)


def _reqs(rng, n):
    return [(int(rng.integers(0, 2)), int(rng.integers(0, ROWS))) for _ in range(n)]


def small_batch(rng, src=5, n=3, cst=0):
    """one message of n requests on one partition"""
    return batch([message(_reqs(rng, n), [0], cst, rng)], src)


def good_cases(seed=7):
    """[(name, batch bytes, txns, accesses)]: every message shape the issue
    names, in batches of every kind."""
    rng = np.random.default_rng(seed)
    out = []
    k = 0
    # requests per txn 0 / 1 / 10 / 128 x partitions per txn 0 / 1 / 4, packed as MessageThread does
    msgs, lens = [], []
    for n in (0, 1, 10, 128):
        for p in (0, 1, 4):
            msgs.append(message(_reqs(rng, n), list(range(p)), 1000 + k, rng))
            lens.append(n)
            k += 1
    pos = 0
    for b in W.batches(NODE, 5, msgs):
        cnt = struct.unpack_from("<I", b, 8)[0]
        out.append((f"shapes{pos}", b, cnt, sum(lens[pos:pos + cnt])))
        pos += cnt
    out.append(("one_message", batch([message(_reqs(rng, 10), [1], 77, rng)], 6), 1, 10))
    b40 = batch([message([], [], 200 + i, rng) for i in range(40)], 7)
    assert len(b40) == 4012
    out.append(("forty_empty", b40, 40, 0))
    # exactly 4,096 bytes: 12 + (100 + 8 + 24 * 128) + (100 + 8 + 24 * 29) + 100
    full = batch([message(_reqs(rng, 128), [3], 300, rng), message(_reqs(rng, 29), [2], 301, rng),
                  message([], [], 302, rng)], 8)
    assert len(full) == 4096
    out.append(("full_4096", full, 3, 157))
    # past lane 64 of the flat loops: 90 partitions in a batch, and (above) 128 requests in a message
    p90 = batch([message([], [i % PART_CNT, 1, 2], 400 + i, rng) for i in range(30)], 9)
    assert len(p90) == 30 * 124 + 12 == 3732
    out.append(("partitions_90", p90, 30, 0))
    out.append(("requests_128", batch([message(_reqs(rng, 128), [0], 500, rng)], 9), 1, 128))
    return out


def malformed_cases(seed=11):
    """[(name, batch bytes, max_req)]: one case of every refusal of
    dv_wire_open (max_req 0: the default limit of 128)."""
    rng = np.random.default_rng(seed)
    ok = lambda n=3, p=(0,): message(_reqs(rng, n), list(p), 9, rng)  # noqa: E731
    m = []
    m.append(("len_below_12", struct.pack("<II", NODE, 5), 0))
    m.append(("len_above_4096", batch([ok(128), ok(40)]) + b"\0" * 100, 0))
    assert len(m[-1][1]) > 4096
    m.append(("dest_not_this_node", batch([ok()], dest=NODE + 1), 0))
    m.append(("src_is_this_node", batch([ok()], src=NODE), 0))
    m.append(("count_zero", batch([], count=0), 0))
    m.append(("count_zero_with_bytes", batch([ok()], count=0), 0))
    m.append(("count_one_more", batch([ok(), ok()], count=3), 0))
    m.append(("count_one_less", batch([ok(), ok()], count=1), 0))
    m.append(("count_huge", batch([ok()], count=0xFFFFFFFF), 0))
    m.append(("trailing_bytes", batch([ok()]) + b"\0" * 8, 0))
    m.append(("truncated_header", batch([ok()])[:12 + 60], 0))
    m.append(("rtype_cl_rsp", batch([ok(), message(_reqs(rng, 2), [0], 1, rng, rtype=W.CL_RSP)]), 0))
    m.append(("rtype_rdone", batch([ok(), W.header(W.RDONE)]), 0))
    m.append(("rdone_shaped_like_a_query", batch([message(_reqs(rng, 2), [0], 1, rng, rtype=W.RDONE)]), 0))
    m.append(("partitions_65", batch([message(_reqs(rng, 1), [0] * 65, 1, rng)]), 0))
    m.append(("partition_out_of_range", batch([ok(), message(_reqs(rng, 4), [0, PART_CNT], 1, rng)]), 0))
    m.append(("requests_129", batch([message(_reqs(rng, 129), [0], 1, rng)]), 0))
    m.append(("requests_above_max_req", batch([message(_reqs(rng, 17), [0], 1, rng)]), 16))
    m.append(("requests_past_the_end", batch([ok(), message(_reqs(rng, 4), [0], 1, rng, n_reqs=5)]), 0))
    m.append(("partitions_past_the_end", batch([message([], [0, 1], 1, rng, n_parts=40)]), 0))
    m.append(("acctype_2", batch([message([(0, 1), (2, 2), (1, 3)], [0], 1, rng)]), 0))
    m.append(("acctype_scan", batch([message([(3, 1)], [0], 1, rng)]), 0))
    m.append(("acctype_high_bits", batch([message([(1 << 8, 1)], [0], 1, rng)]), 0))
    m.append(("key_is_table_size", batch([ok(5), message([(0, ROWS)], [0], 1, rng)]), 0))
    m.append(("key_high_bits", batch([message([(1, 1 << 32)], [0], 1, rng)]), 0))
    # 64-bit counts that wrap n * 24 / n * 8 back into range
    m.append(("requests_wrap_2_61_plus_1", batch([message(_reqs(rng, 1), [0], 1, rng, n_reqs=(1 << 61) + 1)]), 0))
    m.append(("partitions_wrap_2_61", batch([message(_reqs(rng, 1), [], 1, rng, n_parts=1 << 61)]), 0))
    m.append(("requests_2_32_plus_1", batch([message(_reqs(rng, 1), [0], 1, rng, n_reqs=(1 << 32) + 1)]), 0))
    # the twins of good_cases' partitions_90 / requests_128: the bad field past flat index 63 of its loop
    parts = [[0, 1, 2] for _ in range(30)]
    parts[82 // 3][82 % 3] = PART_CNT
    m.append(("partition_82_of_90_out_of_range", batch([message([], p, 1, rng) for p in parts]), 0))
    assert len(m[-1][1]) == 3732
    reqs = _reqs(rng, 128)
    reqs[100] = (reqs[100][0], ROWS)
    m.append(("request_100_of_128_key_is_table_size", batch([message(reqs, [0], 1, rng)]), 0))
    return m


# what an offset array does to batch k (the host decoder has no buf_len: the
# second is the device path's own check)
OFF_CASES = ("off_decreases", "off_past_buf_len")


def stream(batches):
    """batches back to back: (uint8 array, uint64 offsets)"""
    off = np.zeros(len(batches) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in batches])
    return np.frombuffer(b"".join(batches), np.uint8).copy(), off


def host_cfg(max_req=0, **kw):
    d = dict(node_id=NODE, node_cnt=NODE_CNT, part_cnt=PART_CNT, synth_table_size=ROWS, max_req=max_req)
    d.update(kw)
    return d


def host_decode(buf, off, first, last, next_txn=0, max_req=0):
    """batches [first, last) through the host decoder, one epoch (WireEpoch)"""
    w = WireIngress(L.YCSB, 1 << 16, 1 << 20, **host_cfg(max_req))
    w.ep.next_txn = next_txn
    if last > first:
        sub = np.ascontiguousarray(off[first:last + 1])
        assert w.feed_buffer(buf, sub) == []
    return w.take()


def _open(b, max_req=0):
    cfg = L.WireCfg(L.YCSB, 0, NODE, NODE_CNT, PART_CNT, max_req, ROWS, None)
    buf = np.frombuffer(b, np.uint8)
    cur = L.WireCursor()
    return L.lib().dv_wire_open(ctypes.byref(cfg), buf.ctypes.data_as(ctypes.c_void_p), len(buf), ctypes.byref(cur))


def test_good_cases_are_accepted_with_the_expected_counts():
    cases = good_cases()
    assert {c[0] for c in cases} >= {"one_message", "forty_empty", "full_4096"} and len(cases) >= 6
    for name, b, txns, accs in cases:
        assert _open(b) == L.DV_OK, name
        buf, off = stream([b])
        ep = host_decode(buf, off, 0, 1)
        assert (ep.n_txn, ep.n_acc) == (txns, accs), name
    lens = set()
    for name, b, txns, accs in cases:
        buf, off = stream([b])
        lens |= set(np.diff(host_decode(buf, off, 0, 1).txn_begin.astype(np.int64)).tolist())
    assert lens >= {0, 1, 10, 128}


@pytest.mark.parametrize("case", malformed_cases(), ids=lambda c: c[0])
def test_malformed_cases_are_refused_by_the_host_decoder(case):
    name, b, max_req = case
    assert _open(b, max_req) == L.DV_ERR_ARG
    if max_req:  # (it is the limit that refuses it)
        assert _open(b, 0) == L.DV_OK


def test_host_decoder_refuses_a_decreasing_offset():
    rng = np.random.default_rng(3)
    buf, off = stream([small_batch(rng) for _ in range(3)])
    off[2] = off[1] - 1
    w = WireIngress(L.YCSB, 100, 1000, **host_cfg())
    cur, nxt = L.WireCursor(), ctypes.c_uint32(0)
    rc = L.lib().dv_wire_decode_batches(ctypes.byref(w.cfg), buf.ctypes.data_as(ctypes.c_void_p),
                                        off.ctypes.data_as(ctypes.c_void_p), 3, ctypes.byref(cur), ctypes.byref(nxt),
                                        ctypes.byref(w.ep))
    assert rc == L.DV_ERR_ARG and nxt.value == 1 and w.ep.n_txn == 1


def _out(**kw):
    one = 0x1000  # (never dereferenced: every call here is refused before a launch)
    d = dict(max_txn=16, pad_=0, max_acc=160, txn_begin=one, n_acc_dev=one, recs32=one, keys=None, types=None,
             acc_txn=None, owner=None, txn_id=None, client_startts=None, return_node=None)
    d.update(kw)
    return L.WireDevOut(**d)


def _ingest(ctx, cfg, out, buf=0x1000, off=0x1000, res=True):
    r = L.WireDevResult()
    return L.lib().dv_wire_ingest_device(ctx, ctypes.byref(cfg) if cfg is not None else None, buf, 64, off, 1, 0,
                                         ctypes.byref(out) if out is not None else None, 0,
                                         ctypes.byref(r) if res else None)


def refused_arguments():
    """[(name, cfg, out)]: argument sets dv_wire_ingest_device refuses before
    any launch, whatever the context (shared with the GPU test, which passes
    a live one)."""
    good = lambda **kw: L.WireCfg(**{**dict(workload=L.YCSB, calvin=0, node_id=NODE, node_cnt=NODE_CNT,  # noqa: E731
                                           part_cnt=PART_CNT, max_req=0, synth_table_size=ROWS, tpcc=None), **kw})
    return [
        ("calvin", good(calvin=1), _out()),
        ("tpcc", good(workload=L.TPCC), _out()),
        ("recs32_with_a_table_above_2_31", good(synth_table_size=(1 << 31) + 1), _out()),
        ("neither_access_form", good(), _out(recs32=None)),
        ("keys_without_types", good(), _out(keys=0x1000)),
        ("no_txn_begin", good(), _out(txn_begin=None)),
        ("no_n_acc_dev", good(), _out(n_acc_dev=None)),
        ("max_txn_zero", good(), _out(max_txn=0)),
        ("max_txn_above_2_24", good(), _out(max_txn=(1 << 24) + 1)),
        ("part_cnt_zero", good(part_cnt=0), _out()),
        ("node_cnt_zero", good(node_cnt=0), _out()),
    ]


def test_new_entry_points_reject_null_and_unsupported_arguments():
    """DV_ERR_ARG before any device is touched"""
    lib = L.lib()
    cfg = L.WireCfg(L.YCSB, 0, NODE, NODE_CNT, PART_CNT, 0, ROWS, None)
    assert _ingest(None, cfg, _out()) == L.DV_ERR_ARG
    assert _ingest(None, None, None, 0, 0, False) == L.DV_ERR_ARG
    for name, c, o in refused_arguments():
        assert _ingest(None, c, o) == L.DV_ERR_ARG, name
    n = ctypes.c_uint32(7)
    assert lib.dv_wire_reply_fields_device(None, None, 4, None, None, None, None, None, None,
                                           ctypes.byref(n)) == L.DV_ERR_ARG
    assert lib.dv_wire_reply_fields_device(None, None, 0, None, None, None, None, None, None, None) == L.DV_ERR_ARG
    assert lib.dv_epoch_reads_tb_only(None, 1 << 20) == L.DV_ERR_ARG


def test_struct_layouts_of_the_device_ingress_match_the_header(tmp_path):
    import os
    import subprocess
    structs = {"dv_wire_dev_out": L.WireDevOut, "dv_wire_dev_result": L.WireDevResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dvcc.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "sz.c"
    src.write_text("\n".join(lines))
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    subprocess.check_call(["gcc", "-I", inc, str(src), "-o", str(tmp_path / "sz")])
    got = dict(line.split() for line in subprocess.check_output([str(tmp_path / "sz")]).decode().splitlines())
    for name, cls in structs.items():
        assert int(got[name]) == ctypes.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, f"{name}.{f}"
