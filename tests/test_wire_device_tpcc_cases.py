"""The cases of the TPC-C device wire ingress (dv_wire_ingest_device_tpcc),
checked here on the HOST decoder alone: every batch the GPU tests
(tests/test_wire_device_tpcc.py) call good is accepted by dv_wire_open and
decoded with the expected counts, every one they call malformed is refused by
it.  So the GPU tests never compare the device path against a case its
reference would not handle as assumed.  Also the C ABI's struct layout and the
argument checks that need no device.

Layout of a batch and its messages: tests/wire_fmt.py.  A TPC-C CL_QRY of p
partitions and n items is 199 + 8 p + 24 n bytes (header 76, client_startts 8,
partition count 8, body 89 + 24 n + 18), so a 4,096-byte batch holds at most
20 messages; a Payment expands to 3 accesses, a NewOrder to 3 + 2 ol_cnt.
"""
import ctypes
import struct

import numpy as np
import pytest

import wire_fmt as W
from dvcc import _lib as L
from dvcc.wire import WireIngress

NODE, NODE_CNT, PART_CNT = 2, 3, 4
MAX_TXN_CAP = 1 << 23  # dv_wire_tpcc_dev_out::max_txn's upper bound (include/dvcc.h)


def _params(num_wh=4, wh_update=1, part_cnt=3):
    return L.TpccParams(num_wh, 10, 1000, 2000, 15, part_cnt, 2, wh_update, 0.5, 1.0)


# parameter sets: the usual one, Payment reading the warehouse, and 128
# warehouses (custNPKey's 10-bit field overflows past warehouse 102, H8)
PSETS = {"base": _params(), "nowh": _params(wh_update=0), "h8": _params(num_wh=128, part_cnt=5)}

# body offsets (after the 92 fixed bytes and the partition words)
BODY = dict(txn_type=0, w_id=8, d_id=16, c_id=24, d_w_id=32, c_w_id=40, c_d_id=48, c_last=56, h_amount=72,
            by_last_name=80, n=81, items=89)
TAIL = dict(rbk=0, remote=1, ol_cnt=2, o_entry_d=10)  # after the items


def tmsg(q, cst=0, patch=None, item_patch=None):
    """One TPC-C CL_QRY from wire_fmt.tpcc_query, then fields overwritten in
    place: patch {field: value} (rtype, np, a body or tail field; 1-byte
    fields take a byte), item_patch (index, column, value)."""
    b = bytearray(W.tpcc_query(q, cst))
    body = 92 + 8 * len(q.get("parts", []))
    tail = body + 89 + 24 * len(q.get("items", []))
    for k, v in (patch or {}).items():
        if k == "rtype":
            struct.pack_into("<I", b, 0, v)
        elif k == "np":
            struct.pack_into("<Q", b, 84, v)
        elif k == "c_last":
            b[body + 56:body + 72] = v
        elif k == "by_last_name":
            b[body + 80] = v
        elif k in ("rbk", "remote"):
            b[tail + TAIL[k]] = v
        elif k in TAIL:
            struct.pack_into("<Q", b, tail + TAIL[k], v)
        else:
            struct.pack_into("<Q", b, body + BODY[k], v)
    if item_patch is not None:
        i, col, v = item_patch
        struct.pack_into("<Q", b, body + 89 + 24 * i + 8 * col, v)
    return bytes(b)


def batch(msgs, src=5, dest=NODE, count=None):
    return struct.pack("<III", dest, src, len(msgs) if count is None else count) + b"".join(msgs)


def pay(w=1, d=1, c=1, c_w=None, c_d=None, h=100, name=None, parts=(0,), items=(), **more):
    q = dict(txn_type=1, w_id=w, d_id=d, c_id=c, d_w_id=w, c_w_id=w if c_w is None else c_w,
             c_d_id=d if c_d is None else c_d, h_amount=h, parts=list(parts), items=list(items))
    if name is not None:
        q.update(by_last_name=True, c_last=name)
    q.update(more)
    return q


def neworder(items, w=1, d=1, c=1, parts=(0,), **more):
    q = dict(txn_type=2, w_id=w, d_id=d, c_id=c, parts=list(parts), items=list(items), ol_cnt=len(items),
             o_entry_d=2013)
    q.update(more)
    return q


def _items(rng, n, p, home=1):
    """n distinct items, about a third supplied by another warehouse"""
    ids = rng.choice(np.arange(1, p.max_items + 1), n, replace=False)
    return [(int(i), int(rng.integers(1, p.num_wh + 1)) if k % 3 == 1 else home, int(rng.integers(1, 11)))
            for k, i in enumerate(ids)]


def small_batch(rng, pset="base", src=5, cst=0, kind=None):
    """one message: a Payment (by id or by name) or a small NewOrder"""
    p = PSETS[pset]
    kind = int(rng.integers(0, 3)) if kind is None else kind
    w, d, c = int(rng.integers(1, p.num_wh + 1)), int(rng.integers(1, 11)), int(rng.integers(1, 1001))
    if kind == 0:
        q = pay(w, d, c, h=int(rng.integers(1, 5000)))
    elif kind == 1:
        q = pay(w, d, 0, c_w=int(rng.integers(1, p.num_wh + 1)), name=b"BARBAROUGHT", h=int(rng.integers(1, 5000)))
    else:
        q = neworder(_items(rng, 1 + int(rng.integers(0, 6)), p, w), w, d, c)
    return batch([tmsg(q, cst)], src)


def _acc(q):
    return 3 if q["txn_type"] == 1 else 3 + 2 * len(q["items"])


def good_cases(pset="base", seed=7):
    """[(name, batch bytes, txns, accesses)] under PSETS[pset]: every message
    shape the device path has to decode, in batches of every kind."""
    rng = np.random.default_rng(seed)
    p = PSETS[pset]
    W_ = p.num_wh
    out = []
    one = lambda name, q, **kw: out.append((name, batch([tmsg(q, len(out) + 500, **kw)], 6), 1, _acc(q)))  # noqa: E731
    junk = (1 << 64) - 3
    one("pay_by_id", pay(W_, 10, 1000, c_w=1, c_d=1, h=(1 << 56) - 1))
    one("pay_name_0", pay(2, 3, 0, name=b""))
    one("pay_name_1", pay(2, 3, 0, c_w=W_, c_d=7, name=b"A"))
    one("pay_name_15", pay(1, 1, 0, name=b"ABCDEFGHIJKLMNO"))
    one("pay_name_garbage_after_nul", pay(3, 4, 0, name=b"BAR"), patch=dict(c_last=b"BAR\0junk\xff\x80junk!!"))
    one("pay_name_odd_bytes", pay(3, 4, 0, c_w=W_, name=b"@\x80\xffA0z"))
    one("pay_by_last_name_byte_2", pay(1, 2, 0, name=b"OUGHTPRI"), patch=dict(by_last_name=2))
    one("pay_with_3_garbage_items", pay(1, 2, 5, items=[(0, 0, 1 << 60), (junk, junk, junk), (1 << 32, 1 << 33, 0)]))
    one("pay_by_id_unchecked_garbage", pay(1, 2, 5, d_w_id=junk, c_last=b"\xff" * 16, ol_cnt=junk, o_entry_d=junk),
        patch=dict(rbk=0xEE, remote=0x7F))
    one("pay_by_name_unchecked_garbage", pay(1, 2, junk, name=b"ESE", d_w_id=0, ol_cnt=63), patch=dict(rbk=2))
    for n in (1, 5, 15, 62):
        one(f"neworder_{n}", neworder(_items(rng, n, p, 2), 2, 9, 999))
    one("neworder_unchecked_garbage",
        neworder(_items(rng, 4, p, 1), W_, 1, 1, d_w_id=junk, c_w_id=junk, c_d_id=0, c_last=b"\x80" * 16,
                 h_amount=junk, by_last_name=True, o_entry_d=junk), patch=dict(rbk=9, remote=0xFF, by_last_name=0xCC))
    for k in (0, 1, 4, 64):
        one(f"partitions_{k}", pay(1, 1, 1, parts=[i % PART_CNT for i in range(k)]))
        one(f"neworder_partitions_{k}", neworder(_items(rng, 2, p, 1), parts=[(i + 1) % PART_CNT for i in range(k)]))
    out.append(("twenty_payments", batch([tmsg(pay(1 + i % W_, 1 + i % 10, 1 + i, parts=()), 700 + i)
                                          for i in range(20)], 7), 20, 60))
    assert len(out[-1][1]) == 12 + 20 * 199
    # exactly 4,096 bytes: 12 + 4 x 199 + 8 x 3 + 24 x (62 + 62 + 12)
    qs = [neworder(_items(rng, 62, p, 1), parts=()), pay(2, 2, 2, parts=(0, 1, 3)),
          neworder(_items(rng, 62, p, W_), W_, parts=()), neworder(_items(rng, 12, p, 1), parts=())]
    full = batch([tmsg(q, 800 + i) for i, q in enumerate(qs)], 8)
    assert len(full) == 4096
    out.append(("full_4096", full, 4, sum(_acc(q) for q in qs)))
    # a mixed batch, packed as MessageThread does
    qs = [pay(1, 1, 1), neworder(_items(rng, 5, p, 1)), pay(1, 2, 0, name=b"PRESEING"), neworder(_items(rng, 15, p, 2)),
          pay(W_, 5, 77, c_w=1, c_d=2)]
    out.append(("mixed", batch([tmsg(q, 900 + i) for i, q in enumerate(qs)], 9), 5, sum(_acc(q) for q in qs)))
    # past lane 64 of the flat loops: 68 partitions in a batch, 80 items in a batch
    qs = [pay(1 + i % W_, 1 + i % 10, 1 + i, parts=[i % PART_CNT, 1, 2, 3]) for i in range(17)]
    out.append(("partitions_68", batch([tmsg(q, 950 + i) for i, q in enumerate(qs)], 9), 17, 51))
    assert len(out[-1][1]) == 17 * 231 + 12 == 3939
    qs = [neworder(_items(rng, 40, p, 1)), neworder(_items(rng, 40, p, 2), 2)]
    out.append(("items_80", batch([tmsg(q, 970 + i) for i, q in enumerate(qs)], 9), 2, 166))
    assert len(out[-1][1]) == 2 * 1167 + 12 == 2346
    return out


def _ok_msgs(rng, p, n):
    qs = []
    for i in range(n):
        qs.append([pay(1, 1, 1 + i), neworder(_items(rng, 3, p, 1)), pay(1, 2, 0, name=b"ABLE")][i % 3])
    return qs


def malformed_cases(seed=11):
    """[(name, batch bytes)] under PSETS['base']: one case of every refusal of
    dv_wire_open for TPC-C, the malformed message at the first, a middle and
    the last place of a five-message batch (a bad item at the first, a middle
    and the last place of its list); then the batch-level refusals."""
    rng = np.random.default_rng(seed)
    p = PSETS["base"]
    big = (1 << 32) + 1
    kinds = []  # (name, query, kwargs of tmsg) -- item cases take the position
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
    kinds.append(("rtype_rdone", None, {}))
    m = []
    for name, q, kw in kinds:
        for where, pos in (("first", 0), ("middle", 2), ("last", 4)):
            kw2 = dict(kw)
            if "item" in kw2:
                col, v = kw2.pop("item")
                kw2["item_patch"] = ({0: 0, 2: len(q["items"]) // 2, 4: len(q["items"]) - 1}[pos], col, v)
            msgs = [tmsg(x, 40 + i) for i, x in enumerate(_ok_msgs(rng, p, 5))]
            msgs[pos] = W.header(W.RDONE) if q is None else tmsg(q, 9, **kw2)
            m.append((f"{name}_{where}", batch(msgs)))
    ok = lambda: [tmsg(x, 60 + i) for i, x in enumerate(_ok_msgs(rng, p, 3))]  # noqa: E731
    m.append(("one_byte_short", batch(ok())[:-1]))
    m.append(("one_byte_over", batch(ok()) + b"\0"))
    m.append(("count_one_more", batch(ok(), count=4)))
    m.append(("count_one_less", batch(ok(), count=2)))
    m.append(("count_zero", batch(ok(), count=0)))
    m.append(("count_zero_and_no_bytes", batch([], count=0)))
    m.append(("dest_not_this_node", batch(ok(), dest=NODE + 1)))
    m.append(("src_is_this_node", batch(ok(), src=NODE)))
    m.append(("len_above_4096", batch([tmsg(neworder(_items(rng, 62, p, 1))) for _ in range(3)])))
    assert len(m[-1][1]) > 4096
    # the twins of good_cases' partitions_68 / items_80: the bad field past flat index 63 of its loop
    parts = [[0, 1, 2, 3] for _ in range(17)]
    parts[66 // 4][66 % 4] = PART_CNT
    m.append(("partition_66_of_68_out_of_range", batch([tmsg(pay(1, 1, 1 + i, parts=x)) for i, x in enumerate(parts)])))
    assert len(m[-1][1]) == 3939
    m.append(("item_70_of_80_i_id_above_max_items",
              batch([tmsg(neworder(_items(rng, 40, p, 1))),
                     tmsg(neworder(_items(rng, 40, p, 1)), item_patch=(70 - 40, 0, p.max_items + 1))])))
    assert len(m[-1][1]) == 2346
    return m


def stream(batches):
    """batches back to back: (uint8 array, uint64 offsets)"""
    off = np.zeros(len(batches) + 1, np.uint64)
    off[1:] = np.cumsum([len(b) for b in batches])
    return np.frombuffer(b"".join(batches), np.uint8).copy(), off


def wire_cfg(pset="base", **kw):
    d = dict(workload=L.TPCC, calvin=0, node_id=NODE, node_cnt=NODE_CNT, part_cnt=PART_CNT, max_req=0,
             synth_table_size=0, tpcc=ctypes.pointer(PSETS[pset]) if pset else None)
    d.update(kw)
    return L.WireCfg(**d)


def host_decode(buf, off, first, last, next_txn=0, pset="base"):
    """batches [first, last) through the host decoder, one epoch (WireEpoch)"""
    w = WireIngress(L.TPCC, 1 << 14, 1 << 19, node_id=NODE, node_cnt=NODE_CNT, part_cnt=PART_CNT, tpcc=PSETS[pset])
    w.ep.next_txn = next_txn
    if last > first:
        sub = np.ascontiguousarray(off[first:last + 1])
        assert w.feed_buffer(buf, sub) == []
    return w.take()


def _open(b, pset="base"):
    cfg = wire_cfg(pset)
    buf = np.frombuffer(b, np.uint8)
    cur = L.WireCursor()
    return L.lib().dv_wire_open(ctypes.byref(cfg), buf.ctypes.data_as(ctypes.c_void_p), len(buf), ctypes.byref(cur))


@pytest.mark.parametrize("pset", list(PSETS))
def test_good_cases_are_accepted_with_the_expected_counts(pset):
    cases = good_cases(pset)
    names = {c[0] for c in cases}
    assert names >= {"pay_name_odd_bytes", "neworder_62", "partitions_64", "twenty_payments", "full_4096"}
    lens, tables = set(), set()
    for name, b, txns, accs in cases:
        assert _open(b, pset) == L.DV_OK, name
        buf, off = stream([b])
        ep = host_decode(buf, off, 0, 1, pset=pset)
        assert (ep.n_txn, ep.n_acc) == (txns, accs), name
        lens |= set(np.diff(ep.txn_begin.astype(np.int64)).tolist())
        tables |= set(ep.tables.tolist())
    assert lens >= {3, 5, 13, 33, 127} and tables == {0, 1, 2, 3, 4, 5}
    assert max(len(c[1]) for c in cases) == 4096


def test_the_parameter_sets_differ_where_they_should():
    buf, off = stream([c[1] for c in good_cases("base")])
    a, b = host_decode(buf, off, 0, len(off) - 1), host_decode(buf, off, 0, len(off) - 1, pset="nowh")
    assert (a.types != b.types).any() and (a.args != b.args).any() and (a.keys == b.keys).all()
    # H8: a by-name key of a warehouse past 102 carries into the name's bits
    h8 = dict((c[0], c) for c in good_cases("h8"))["pay_name_1"]
    ep = host_decode(*stream([h8[1]]), 0, 1, pset="h8")
    assert ep.tables[2] == L.T_CUST_LAST and int(ep.keys[2]) == 128 * 10 + 7 and int(ep.keys[2]) >> 10 == 1
    assert len(set(ep.owner.tolist())) > 1


@pytest.mark.parametrize("case", malformed_cases(), ids=lambda c: c[0])
def test_malformed_cases_are_refused_by_the_host_decoder(case):
    name, b = case
    assert _open(b) == L.DV_ERR_ARG


def test_malformed_cases_differ_from_a_good_batch_only_where_named():
    """the five-message batches without their patch are accepted: it is the
    named field that refuses each, not the builder"""
    rng = np.random.default_rng(11)
    p = PSETS["base"]
    for pos in (0, 2, 4):
        msgs = [tmsg(x, 40 + i) for i, x in enumerate(_ok_msgs(rng, p, 5))]
        msgs[pos] = tmsg(neworder(_items(rng, 5, p, 1)), 9, item_patch=(2, 2, (1 << 56) - 1))
        assert _open(batch(msgs)) == L.DV_OK
    assert _open(batch([tmsg(pay(h=(1 << 56) - 1)), tmsg(pay(1, 1, 0, name=b"ABCDEFGHIJKLMNO"))])) == L.DV_OK
    assert _open(batch([tmsg(neworder([(1 + i, 1, 1) for i in range(62)]))])) == L.DV_OK


def _out(**kw):
    one = 0x1000  # (never dereferenced: every call here is refused before a launch)
    d = dict(max_txn=16, pad_=0, max_acc=160, txn_begin=one, n_acc_dev=one, keys=one, types=one, acc_txn=one,
             tables=one, args=one, txn_type=None, owner=None, txn_id=None, client_startts=None, return_node=None)
    d.update(kw)
    return L.WireTpccDevOut(**d)


def _ingest(ctx, cfg, out, buf=0x1000, off=0x1000, res=True, n_batches=1, first=0):
    r = L.WireDevResult(status=77)
    rc = L.lib().dv_wire_ingest_device_tpcc(ctx, ctypes.byref(cfg) if cfg is not None else None, buf, 64, off,
                                            n_batches, first, ctypes.byref(out) if out is not None else None, 0,
                                            ctypes.byref(r) if res else None)
    assert r.status == 77  # (*res untouched)
    return rc


def refused_arguments():
    """[(name, cfg, out)]: argument sets dv_wire_ingest_device_tpcc refuses
    before any launch, whatever the context (shared with the GPU test, which
    passes a live one)."""
    bad = lambda **kw: ctypes.pointer(L.TpccParams(**{**dict(  # noqa: E731
        num_wh=4, dist_per_wh=10, cust_per_dist=1000, max_items=2000, max_items_per_txn=15, part_cnt=3,
        part_per_txn=2, wh_update=1, perc_payment=0.5, mpr=1.0), **kw}))
    r = [
        ("calvin", wire_cfg(calvin=1), _out()),
        ("ycsb", wire_cfg(workload=L.YCSB), _out()),
        ("no_params", wire_cfg(None), _out()),
        ("params_cust_per_dist_999", wire_cfg(tpcc=bad(cust_per_dist=999)), _out()),
        ("params_part_cnt_above_num_wh", wire_cfg(tpcc=bad(part_cnt=5)), _out()),
        ("params_no_warehouse", wire_cfg(tpcc=bad(num_wh=0, part_cnt=0)), _out()),
        ("params_items_per_txn_63", wire_cfg(tpcc=bad(max_items_per_txn=63)), _out()),
        ("max_txn_zero", wire_cfg(), _out(max_txn=0)),
        ("max_txn_above_the_cap", wire_cfg(), _out(max_txn=MAX_TXN_CAP + 1)),
        ("part_cnt_zero", wire_cfg(part_cnt=0), _out()),
        ("node_cnt_zero", wire_cfg(node_cnt=0), _out()),
    ]
    for f in ("txn_begin", "n_acc_dev", "keys", "types", "acc_txn", "tables", "args"):
        r.append((f"no_{f}", wire_cfg(), _out(**{f: None})))
    return r


def test_the_new_entry_point_rejects_null_and_unsupported_arguments():
    """DV_ERR_ARG before any device is touched"""
    cfg = wire_cfg()
    assert _ingest(None, cfg, _out()) == L.DV_ERR_ARG
    assert _ingest(None, None, None, 0, 0, False) == L.DV_ERR_ARG
    assert _ingest(None, cfg, _out(), n_batches=1, first=2) == L.DV_ERR_ARG
    for name, c, o in refused_arguments():
        assert _ingest(None, c, o) == L.DV_ERR_ARG, name
    # the YCSB entry goes on refusing TPC-C
    r = L.WireDevResult()
    o = L.WireDevOut(16, 0, 160, 0x1000, 0x1000, 0x1000, None, None, None, None, None, None, None)
    assert L.lib().dv_wire_ingest_device(None, ctypes.byref(cfg), 0x1000, 64, 0x1000, 1, 0, ctypes.byref(o), 0,
                                         ctypes.byref(r)) == L.DV_ERR_ARG


def test_struct_layout_of_the_tpcc_device_ingress_matches_the_header(tmp_path):
    import os
    import subprocess
    structs = {"dv_wire_tpcc_dev_out": L.WireTpccDevOut, "dv_wire_dev_result": L.WireDevResult}
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
