"""The CALVIN sequencer on the GPU under a TPC-C cfg (dv_wire_sequence_device,
dv_wire_sequence_acks_device) against the host functions, which
tests/test_wire_sequence_tpcc_cpu.py pins against the independent model --
never against the device path itself.  A TPC-C message is 3 mod 4 bytes, so
mbuf headers, messages and RDONEs start at any byte of `out` and neighbours
share dwords: every output is pre-filled, every case runs with the fills 0x00
and 0xFF (an unwritten byte cannot hide behind a matching fill), and the fill
must stand from n_bytes to the tensor's end.  The tile sizes are read from
the source, as tests/test_wire_sequence_cases_gpu.py reads them.
"""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import _oracle as O
import wire_fmt as W
import wire_seq as S
import wire_seq_tpcc as ST

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc import tpcc as T  # noqa: E402
from dvcc import wire as DW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LAYOUT = open(os.path.join(ROOT, "deneva-plus_amd", "csrc", "dvcc_wire_layout.h")).read()
PAD = 64
FILLS = (0x00, 0xFF)


def _const(name):
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*([0-9* ]+);" % name, _LAYOUT)
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f)
    return v


WAVE, CHUNK, TILE = _const("kWireWave"), _const("kWireChunk"), _const("kSeqTile")
assert (WAVE, CHUNK, TILE) == (4, 3072, 256)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    e = dvcc.CCEngine(dvcc.CALVIN, 8192, 1 << 17)
    yield e
    e.close()


def params(t):
    return T.tpcc_params(t["num_wh"], t["dist"], t["cust"], t["items"], part_cnt=t["part_cnt"])


def filled(n, dt, fill, lead=0):
    """n elements of dt behind `lead` bytes, PAD elements more, every byte `fill` -> (the whole tensor, its view at lead)"""
    size = torch.empty(0, dtype=dt).element_size()
    t = torch.full((lead + (n + PAD) * size,), fill, dtype=torch.uint8, device="cuda")
    return t, t[lead:].view(dt)


def upload(buf, off, shift=0):
    """the queue `shift` bytes into a 64-byte aligned tensor"""
    t = torch.zeros(shift + len(buf) + 64, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 64 == 0
    t[shift:shift + len(buf)] = torch.from_numpy(buf)
    return t[shift:], torch.from_numpy(off.view(np.int64)).cuda()


def host_sequence(mbufs, batch_id, k, first=0, **extra):
    buf, off = S.queue(mbufs)
    return DW.sequence_host(buf, off, batch_id, node_id=k["node_id"], node_cnt=k["node_cnt"], part_cnt=k["part_cnt"],
                            n_dest=k["n_dest"], max_txn=k["max_txn"], first_batch=first, params=params(k["tp"]),
                            **extra)


def same_or_fill(name, dev, ref, n, fill):
    """dev (a pre-filled device view) holds ref[:n] and its fill behind it"""
    h = dev.cpu().numpy().view(ref.dtype)
    bad = np.flatnonzero(h[:n] != ref[:n])
    assert bad.size == 0, f"{name} (fill {fill:#x}): first difference at {bad[:4]} of {n}"
    assert (h[n:].view(np.uint8) == fill).all(), f"{name} (fill {fill:#x}): written past {n}"


def sequence_and_check(eng, mbufs, batch_id, k, first=0, cap=None, max_batches=None, shift=0, ref=None, fills=FILLS):
    """The device call over pre-filled outputs, once per fill, against the host
    function with the same capacities: the result record, every output, the
    fill behind what was written (everywhere, on a refused call).  Returns the
    host's SequencedBatch."""
    buf, off = S.queue(mbufs)
    ref = host_sequence(mbufs, batch_id, k, first, cap=cap, max_batches=max_batches) if ref is None else ref
    room = DW._seq_room(len(buf), k["node_cnt"])
    cap, max_b = room[0] if cap is None else cap, room[1] if max_batches is None else max_batches
    d_buf, d_off = upload(buf, off, shift)
    T_ = k["max_txn"]
    pp = params(k["tp"])
    cfg = DW._seq_cfg(k["node_id"], k["node_cnt"], k["part_cnt"], 0, 0, pp)
    r = ref.result
    for fill in fills:
        whole, out = filled(max(cap, 4), torch.uint8, fill)
        _, boff = filled(max_b + 1, torch.int64, fill)
        _, dfirst = filled(k["node_cnt"] + 1, torch.int32, fill)
        _, wc = filled(T_, torch.int32, fill)
        _, ws = filled(T_, torch.int64, fill)
        _, wa = filled(T_, torch.int32, fill)
        sin = L.WireSeqIn(d_buf.data_ptr(), len(buf), d_off.data_ptr(), len(mbufs), first, batch_id, k["n_dest"], T_)
        sout = L.WireSeqOut(out.data_ptr(), cap, boff.data_ptr(), max_b, 0, dfirst.data_ptr(), wc.data_ptr(),
                            ws.data_ptr(), wa.data_ptr())
        res = L.WireSeqResult(status=77)
        eng._after_torch()
        rc = L.lib().dv_wire_sequence_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(sin), ctypes.byref(sout),
                                             ctypes.byref(res))
        torch.cuda.synchronize()
        got = (rc, res.status, res.n_taken, res.n_txn, res.n_out, res.n_msgs, res.n_bytes)
        assert got == (r.status, r.status, r.n_taken, r.n_txn, r.n_out, r.n_msgs, r.n_bytes), (got, r.n_bytes, r.n_out)
        refused = r.n_bytes > cap or r.n_out > max_b
        same_or_fill("out", out, ref.out, 0 if refused else r.n_bytes, fill)
        same_or_fill("batch_off", boff, ref.batch_off, 0 if refused else r.n_out + 1, fill)
        same_or_fill("dest_first", dfirst, ref.dest_first, 0 if refused else k["node_cnt"] + 1, fill)
        n = 0 if refused else r.n_txn
        same_or_fill("wait_client", wc, ref.wait_client, n, fill)
        same_or_fill("wait_startts", ws, ref.wait_startts, n, fill)
        same_or_fill("wait_acks", wa, ref.wait_acks, n, fill)
    return ref


# ---- the CPU suite's cases
CASES = ST.sequence_cases()


@pytest.mark.parametrize("name,mbufs,batch_id,k", CASES, ids=[c[0] for c in CASES])
def test_sequence_equals_the_host_function(eng, name, mbufs, batch_id, k):
    ref = sequence_and_check(eng, mbufs, batch_id, k)
    assert ref.result.status == L.DV_OK and ref.result.n_taken == len(mbufs)


FILL_CASES = ST.fill_cases()


@pytest.mark.parametrize("name,mbufs,batch_id,k,n_out,last", FILL_CASES, ids=[c[0] for c in FILL_CASES])
def test_an_mbuf_filled_to_the_byte_and_eight_bytes_over(eng, name, mbufs, batch_id, k, n_out, last):
    ref = sequence_and_check(eng, mbufs, batch_id, k)
    assert ref.result.n_out == n_out and len(ref.mbufs()[-1]) == last


def test_max_txn_cap_and_max_batches_at_their_edges(eng):
    by = {c[0]: c for c in CASES}
    _, mbufs, e, k = by["two_nodes"]
    n = host_sequence(mbufs, e, k).result.n_txn
    for max_txn, status in ((n, L.DV_OK), (n - 1, L.WIRE_MORE), (1, L.DV_ERR_ARG)):
        assert sequence_and_check(eng, mbufs, e, dict(k, max_txn=max_txn)).result.status == status
    kk = dict(k, max_txn=n - 1)
    first = host_sequence(mbufs, e, kk).result.n_taken
    assert sequence_and_check(eng, mbufs, e + 1, kk, first=first).result.status == L.DV_OK
    _, mbufs, e, k = by["mixed_cuts"]
    free = host_sequence(mbufs, e, k).result
    assert sequence_and_check(eng, mbufs, e, k, cap=free.n_bytes, max_batches=free.n_out).result.status == L.DV_OK
    for extra in (dict(cap=free.n_bytes - 1), dict(max_batches=free.n_out - 1)):
        assert sequence_and_check(eng, mbufs, e, k, **extra).result.status == L.DV_ERR_ARG  # (every output keeps its fill)


MALFORMED = ST.malformed_cases()


@pytest.mark.parametrize("name,mbufs,k,n_taken,stamped", MALFORMED, ids=[c[0] for c in MALFORMED])
def test_a_malformed_mbuf_stops_the_batch(eng, name, mbufs, k, n_taken, stamped):
    ref = sequence_and_check(eng, mbufs, 4, k)
    accepted = name == "payment_items_unchecked"
    assert ref.result.status == (L.DV_OK if accepted else L.DV_ERR_ARG) and ref.result.n_taken == n_taken


def test_a_tpcc_cfg_without_its_params_is_refused_and_with_them_taken(eng):
    k = ST.kw(node_cnt=2, part_cnt=2, tp_=ST.tp(part_cnt=2))
    mbufs = [W.batches(0, 2, [ST.payment(1, 2)])[0]]
    buf, off = S.queue(mbufs)
    d_buf, d_off = upload(buf, off)
    outs = [filled(n, dt, 0xA5)[1] for n, dt in ((4096, torch.uint8), (8, torch.int64), (8, torch.int32),
                                                 (8, torch.int32), (8, torch.int64), (8, torch.int32))]
    sin = L.WireSeqIn(d_buf.data_ptr(), len(buf), d_off.data_ptr(), 1, 0, 5, 4, 8)
    sout = L.WireSeqOut(outs[0].data_ptr(), 4096, outs[1].data_ptr(), 4, 0, *[t.data_ptr() for t in outs[2:]])
    ain = L.WireSeqAckIn(d_buf.data_ptr(), len(buf), d_off.data_ptr(), 1, 4, 5, 2, 0, outs[3].data_ptr(),
                         outs[4].data_ptr(), outs[5].data_ptr())
    rout = L.WireRspOut(outs[0].data_ptr(), 4096, outs[1].data_ptr(), 4, 0)
    pp, wrong = params(k["tp"]), T.tpcc_params(4, part_cnt=5)  # (more partitions than warehouses: knobs refused)
    eng._after_torch()
    for p in (None, wrong):
        cfg = L.WireCfg(L.TPCC, 1, 0, 2, 2, 0, 0, ctypes.pointer(p) if p is not None else None)
        res, ares = L.WireSeqResult(status=77), L.WireSeqAckResult(status=77)
        assert L.lib().dv_wire_sequence_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(sin), ctypes.byref(sout),
                                               ctypes.byref(res)) == L.DV_ERR_ARG and res.status == 77
        assert L.lib().dv_wire_sequence_acks_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(ain), ctypes.byref(rout),
                                                    ctypes.byref(ares)) == L.DV_ERR_ARG and ares.status == 77
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.uint8) == 0xA5).all() for t in outs)
    cfg = DW._seq_cfg(0, 2, 2, 0, 0, pp)
    res = L.WireSeqResult(status=77)
    assert L.lib().dv_wire_sequence_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(sin), ctypes.byref(sout),
                                           ctypes.byref(res)) == L.DV_OK and (res.n_txn, res.n_msgs) == (1, 2)
    torch.cuda.synchronize()


# ---- byte granularity
def _starts(b, node_cnt):
    """(mbuf header starts, message starts, RDONE starts) in out, from the host's offsets and the bytes themselves"""
    hdrs, msgs, rdones = [], [], []
    for j in range(b.result.n_out):
        lo, hi = int(b.batch_off[j]), int(b.batch_off[j + 1])
        hdrs.append(lo)
        at = lo + 12
        for _ in range(struct.unpack_from("<I", b.out, lo + 8)[0]):
            (rtype,) = struct.unpack_from("<I", b.out, at)
            if rtype == W.RDONE:
                rdones.append(at)
                at += 84
            else:
                np_ = struct.unpack_from("<Q", b.out, at + 92)[0]
                n = struct.unpack_from("<Q", b.out, at + 100 + 8 * np_ + 81)[0]
                msgs.append((at, ST.size(np_, n), struct.unpack_from("<Q", b.out, at + 4)[0]))
                at += ST.size(np_, n)
        assert at == hi
    return hdrs, msgs, rdones


def alignment_case():
    t = ST.tp(num_wh=32, part_cnt=16)
    k = ST.kw(node_id=2, node_cnt=16, part_cnt=16, tp_=t, n_dest=20, max_txn=512)
    rng = np.random.default_rng(5)
    msgs = ST.random_txns(rng, 200, 16, t, nps=(0, 1, 2, 3), ns=(1, 2, 5, 15, 40))
    return [W.batches(2, 16 + i % 4, [m])[0] for i, m in enumerate(msgs)], k


def test_every_residue_mod_4_and_dwords_shared_between_waves(eng):
    """Sixteen nodes, one Payment or NewOrder per client mbuf (a wave each), so
    that neighbours in a destination's list come from different waves and
    workgroups.  From the host's offsets: message starts, mbuf header starts
    and RDONE starts each take all four residues mod 4, and two entries
    written for different client mbufs share a dword.  Then the device equals
    the host with the input at 8 byte offsets of a 64-byte line."""
    mbufs, k = alignment_case()
    ref = host_sequence(mbufs, 17, k)
    assert ref.result.status == L.DV_OK
    hdrs, ms, rdones = _starts(ref, 16)
    assert {x % 4 for x in hdrs} == {x % 4 for x, _, _ in ms} == {x % 4 for x in rdones} == {0, 1, 2, 3}
    # consecutive messages of one mbuf: txn k and txn k' from client mbufs k / 5 and k' / 5 (one txn per client mbuf)
    shared = [(a, c) for a, c in zip(ms, ms[1:]) if a[0] + a[1] == c[0] and c[0] % 4 and a[2] != c[2]]
    assert len(shared) >= 10
    for shift in (0, 1, 2, 3, 5, 16, 31, 63):
        sequence_and_check(eng, mbufs, 17, k, shift=shift, ref=ref)


# ---- edges of the machinery
@pytest.mark.parametrize("nb", [WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_client_mbuf_counts_at_the_wave_and_the_scan_chunk(eng, nb):
    """a Payment (two nodes of three) or a one-item NewOrder per client mbuf; one mbuf malformed at the end, and max_txn one short"""
    t = ST.tp(num_wh=6, part_cnt=3)
    k = ST.kw(node_cnt=3, part_cnt=3, tp_=t, max_txn=nb + 8, n_dest=6)
    mbufs = [W.batches(0, 3 + b % 3, [ST.payment(1 + b % 6, 1 + (b // 2) % 6, cst=b) if b % 2 else
                                      ST.new_order(1 + b % 6, [(1 + b, 1 + (b // 3) % 6, 2)], cst=b)])[0]
             for b in range(nb)]
    sequence_and_check(eng, mbufs, 30, k)
    sequence_and_check(eng, mbufs[:-1] + [mbufs[-1][:-1]], 30, k, fills=(0xFF,))
    sequence_and_check(eng, mbufs, 30, dict(k, max_txn=nb - 1), fills=(0x00,))


@pytest.mark.parametrize("size", [215, 1703])
@pytest.mark.parametrize("n_msgs", [TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 2 * TILE + 16])
def test_list_lengths_at_the_cut_searchs_tile(eng, n_msgs, size):
    """A destination's list (its messages and the RDONE) around one and two
    tiles of the cut search: 215-byte Payments, 18 to an mbuf (19 are one
    byte too many), and 1,703-byte NewOrders, 2 to an mbuf: with those an
    mbuf opens on entry 256, the first of the second tile."""
    per = (4096 - 12) // size
    assert per == (18 if size == 215 else 2) and 19 * 215 == 4096 - 12 + 1
    k = ST.kw(max_txn=3 * TILE, tp_=ST.tp(num_wh=4))
    ref = sequence_and_check(eng, ST.sized_queue(n_msgs, size), 31, k)
    assert per * size + 84 <= 4096 - 12  # (a full mbuf of either size has 84 bytes left for the RDONE)
    assert ref.result.n_out == (n_msgs + per - 1) // per


def test_a_tile_of_lone_messages_the_longest_jump(eng):
    """messages above 2,042 bytes: every entry opens an mbuf, the longest walk inside a tile"""
    big = [ST.new_order(1 + i % 4, [(1 + j, 1 + j % 4, j) for j in range(62)], cst=i, parts=[0] * 44)
           for i in range(TILE + 40)]
    assert len(big[0]) == ST.size(44, 62) == 2047 and len(big[0]) > (4096 - 12) // 2
    k = ST.kw(max_txn=2 * TILE, tp_=ST.tp(num_wh=4))
    # (an mbuf each; the 84-byte RDONE still fits behind the last: 2,047 + 84 <= 4,084)
    assert sequence_and_check(eng, ST.clients(big, 0, 1), 32, k).result.n_out == TILE + 40


def _encode(qs, n, cst0=0):
    """dv_tpcc_gen_queries' queries as clients' CL_QRYs of a CALVIN build"""
    msgs = []
    for i in range(n):
        x = qs[i]
        msgs.append(ST.query(dict(
            txn_type=x.txn_type, w_id=x.w_id, d_id=x.d_id, c_id=x.c_id, d_w_id=x.d_w_id, c_w_id=x.c_w_id,
            c_d_id=x.c_d_id, c_last=bytes(x.c_last), h_amount=x.h_amount, by_last_name=x.by_last_name,
            ol_cnt=x.ol_cnt, o_entry_d=x.o_entry_d, rbk=x.rbk, remote=x.remote,
            parts=[x.parts[j] for j in range(x.n_parts)],
            items=[(x.items[j].ol_i_id, x.items[j].ol_supply_w_id, x.items[j].ol_quantity) for j in range(x.ol_cnt)]),
            cst0 + 3 * i))
    return msgs


def test_twenty_thousand_generated_txns_over_five_nodes(eng):
    n = 20_000
    t = ST.tp(num_wh=16, part_cnt=8)
    pp = params(t)
    msgs = _encode(DW.tpcc_gen_queries(pp, n, 23), n)
    k = ST.kw(node_id=3, node_cnt=5, part_cnt=8, tp_=t, n_dest=9, max_txn=n)
    ref = sequence_and_check(eng, ST.clients(msgs, 3, 5, 4, per=9), 33, k)
    assert ref.result.status == L.DV_OK and ref.result.n_txn == n and ref.result.n_msgs > n


# ---- round trips
def _expand(pp, qs, idx):
    """dv_tpcc_expand of the queries qs[i], i in idx -> (keys, types, tables, args, txn_begin)"""
    sel = (L.TpccQuery * max(1, len(idx)))(*[qs[i] for i in idx])
    cap = max(1, len(idx)) * (3 + 2 * L.TPCC_MAX_OL)
    keys, args = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    types, tables = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    tb = np.zeros(len(idx) + 1, np.uint32)
    p = lambda a: a.ctypes.data  # noqa: E731
    L.check(L.lib().dv_tpcc_expand(ctypes.byref(pp), sel, len(idx), cap, p(keys), p(types), p(tables), p(args), p(tb),
                                   None, None), "dv_tpcc_expand")
    a = int(tb[-1])
    return keys[:a], types[:a], tables[:a], args[:a], tb


def _participants(x, t, node_cnt):
    whs = [x.w_id] + ([x.c_w_id] if x.txn_type == 1 else [x.items[j].ol_supply_w_id for j in range(x.ol_cnt)])
    return {((w - 1) % t["part_cnt"]) % node_cnt for w in whs}


def _stream_of(out, boff, dfirst, d):
    """destination d's mbufs, in device memory as they are: (bytes view, their offsets from its first)"""
    h_off = boff.cpu().numpy().view(np.uint64)
    first = dfirst.cpu().numpy().view(np.uint32).tolist()
    lo, hi = int(h_off[first[d]]), int(h_off[first[d + 1]])
    rel = (h_off[first[d]:first[d + 1] + 1] - h_off[first[d]]).view(np.int64)
    return out[lo:hi], torch.from_numpy(rel.copy()).cuda()


def test_each_destinations_stream_decodes_to_its_txns(eng):
    """A generated batch sequenced for 2 nodes; destination d's mbufs, as they
    lie in device memory (at whatever byte), into a CalvinTpccDeviceWireIngress
    of node d: the txn ids are node_id + 2 k of exactly the txns with d among
    their participants, in order, and the access lists dv_tpcc_expand's of
    those queries.  An ingest refuses a stream from its own node, so
    destination d is fed from the sequencer of the other node.  (A generated
    query's w_id lies on its home partition: half the queries are at home on
    partition 0, node 0, half on partition 1, node 1.)"""
    n, E = 1500, 8
    t = ST.tp(num_wh=8, part_cnt=4)
    pp = params(t)
    halves = [DW.tpcc_gen_queries(pp, n // 2, 31 + h, home_part=h) for h in (0, 1)]
    qs = [halves[i % 2][i // 2] for i in range(n)]
    mbufs = ST.clients(_encode(qs, n, cst0=9000), 0, 2, 3, per=11)
    mbufs_of = lambda node: [struct.pack("<I", node) + b[4:] for b in mbufs]  # noqa: E731
    for d in (0, 1):
        seq_node = 1 - d
        seq = dvcc.DeviceSequencer(eng, node_id=seq_node, node_cnt=2, part_cnt=4, synth_table_size=0, max_req=0,
                                   max_txn=n, n_dest=5, params=pp)
        buf, off = S.queue(mbufs_of(seq_node))
        out, boff, dfirst, res = seq.sequence(buf, off, E)
        assert (res.status, res.n_taken, res.n_txn) == (L.DV_OK, len(mbufs), n)
        torch.cuda.synchronize()
        mine = [i for i in range(n) if d in _participants(qs[i], t, 2)]
        assert 0 < len(mine) < n
        s_buf, s_off = _stream_of(out, boff, dfirst, d)
        ing = DW.CalvinTpccDeviceWireIngress(eng, pp, n, 130 * n, node_id=d, node_cnt=2, part_cnt=4)
        dep, _ = ing.sequence([(s_buf, s_off)])
        torch.cuda.synchronize()
        keys, types, tables, args, tb = _expand(pp, qs, mine)
        assert (dep.n_txn, dep.n_acc, dep.rdone, dep.batch_id) == (len(mine), len(keys), 1, E)
        assert dep.txn_id.cpu().numpy().view(np.uint64).tolist() == [seq_node + 2 * i for i in mine]
        assert (dep.client_startts.cpu().numpy().view(np.uint64) == 9000 + 3 * np.array(mine)).all()
        assert (dep.txn_begin.cpu().numpy().view(np.uint32) == tb).all()
        assert (dep.keys.cpu().numpy().view(np.uint64) == keys).all() and (dep.types.cpu().numpy() == types).all()
        assert (dep.tables.cpu().numpy() == tables).all() and (dep.args.cpu().numpy().view(np.uint64) == args).all()


def test_one_batch_end_to_end_on_one_gpu():
    """Clients' TPC-C mbufs -> DeviceSequencer (node 1 of 2; one TPC-C
    partition, so every txn's participant is node 0 alone: the one-node run,
    with a sequencer the ingest accepts a stream from) -> node 0's stream into
    a CALVIN TPC-C ingest -> the epoch run by a CALVIN TpccEngine against the
    oracle -> respond_device's CALVIN_ACKs -> DeviceSequencer.acks: one CL_RSP
    per txn to its client with its client_startts, no ack outstanding."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    n, E, kw = 600, 6, dict(num_wh=4, cust_per_dist=1000, max_items=2000)
    pp, po = T.tpcc_params(**kw), O.tpcc_params(**kw)
    qs = DW.tpcc_gen_queries(pp, n, 77)
    mbufs = ST.clients(_encode(qs, n, cst0=5000), 1, 2, n_clients=3, per=7)
    client_of = [c for b in mbufs for c in [int.from_bytes(b[4:8], "little")] * int.from_bytes(b[8:12], "little")]
    db = O.TpccDB(po, 5)
    eng = T.TpccEngine(dvcc.CALVIN, pp, n, seed=5)
    try:
        seq = dvcc.DeviceSequencer(eng, node_id=1, node_cnt=2, part_cnt=1, synth_table_size=0, max_req=0, max_txn=n,
                                   n_dest=5, params=pp)
        buf, off = S.queue(mbufs)
        out, boff, dfirst, res = seq.sequence(buf, off, E)
        assert (res.status, res.n_taken, res.n_txn, res.n_msgs) == (L.DV_OK, len(mbufs), n, n)
        torch.cuda.synchronize()
        own, _ = _stream_of(out, boff, dfirst, 1)
        assert own.cpu().numpy().tobytes() == W.batches(1, 1, [W.rdone(E)])[0]  # node 1's own stream: the RDONE alone
        s_buf, s_off = _stream_of(out, boff, dfirst, 0)
        ing = DW.CalvinTpccDeviceWireIngress(eng, pp, n, 33 * n, node_id=0, node_cnt=2)
        dep, _ = ing.sequence([(s_buf, s_off)])
        keys, types, tables, args, tb = _expand(pp, qs, list(range(n)))
        assert (dep.n_txn, dep.n_acc, dep.rdone, dep.batch_id) == (n, len(keys), 1, E)
        c_ref, o_ref, st_ref = db.epoch(O.CALVIN, keys, types, tables, args, tb)
        assert c_ref.all() and st_ref.committed == n  # (CALVIN aborts none: on the oracle first)
        d_commit = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_oid = torch.zeros(n, dtype=torch.int64, device="cuda")
        st = eng.run_tpcc_epoch_device(dep, dep.args, d_commit, d_oid)
        assert (d_commit.cpu().numpy() == c_ref).all() and st.committed == n
        assert (d_oid.cpu().numpy().view(np.uint64) == o_ref).all()
        assert (dep.txn_id.cpu().numpy().view(np.uint64) == 1 + 2 * np.arange(n)).all()
        ing.n_dest = 2
        a_out, a_off, a_n = ing.respond_device(dep)
        r_out, r_off, r_n, ares = seq.acks(a_out, a_off)
        assert (ares.status, ares.n_acks, ares.n_skipped, ares.n_done) == (L.DV_OK, n, 0, n)
        torch.cuda.synchronize()
        assert not seq.wait_acks[:n].cpu().numpy().any()
        answered = {}
        for b in DW.reply_batches(r_out, r_off, r_n):
            dest, src, rs = S.parse_rsp_mbuf(b)
            assert src == 1
            for tid, bid, c in rs:
                assert bid == W.U64_MAX and tid % 2 == 1 and tid // 2 not in answered
                answered[tid // 2] = (dest, c)
        assert answered == {i: (client_of[i], 5000 + 3 * i) for i in range(n)}
        for tab_id in range(5):
            tab = db.table(tab_id)
            for col in range(3):
                assert (eng.read_col(tab_id, col) == tab[1 + col]).all(), f"table {tab_id} col {col}"
    finally:
        eng.close()


# ---- the acks and the other workload on the same context
def test_acks_under_a_tpcc_cfg_equal_the_host_function(eng):
    """the acks of tests/wire_seq.py's cases, call after call, under a TPC-C cfg: the host function's outputs"""
    pp = T.tpcc_params(4, part_cnt=2)
    for name, wait, batch_id, calls, k in S.ack_cases():
        wc = np.array([w[0] for w in wait], np.uint32)
        ws = np.array([w[1] for w in wait], np.uint64)
        h_wa = np.array([w[2] for w in wait], np.uint32)
        n = len(wait)
        _, d_wa = filled(n, torch.int32, 0xFF)
        d_wa[:n] = torch.from_numpy(h_wa.view(np.int32))
        d_wc, d_ws = torch.from_numpy(wc.view(np.int32)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
        cfg = DW._seq_cfg(k["node_id"], k["node_cnt"], 1, 0, 0, pp)
        for mbufs in calls:
            buf, off = S.queue(mbufs)
            h_out, h_off, r = DW.sequence_acks_host(buf, off, batch_id, wc, ws, h_wa, params=pp, **k)
            cap, max_b = DW._seq_rsp_room(n, k["n_dest"])
            d_buf, d_off = upload(buf if len(buf) else np.zeros(1, np.uint8), off)
            _, out = filled(max(cap, 4), torch.uint8, 0xFF)
            _, boff = filled(max_b + 1, torch.int64, 0xFF)
            ain = L.WireSeqAckIn(d_buf.data_ptr(), len(buf), d_off.data_ptr(), len(mbufs), k["n_dest"], batch_id, n, 0,
                                 d_wc.data_ptr(), d_ws.data_ptr(), d_wa.data_ptr())
            rout = L.WireRspOut(out.data_ptr(), cap, boff.data_ptr(), max_b, 0)
            res = L.WireSeqAckResult(status=77)
            eng._after_torch()
            rc = L.lib().dv_wire_sequence_acks_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(ain), ctypes.byref(rout),
                                                      ctypes.byref(res))
            torch.cuda.synchronize()
            got = (rc, res.status, res.first_bad, res.n_acks, res.n_skipped, res.n_done, res.n_batches, res.n_bytes)
            assert got == (r.status, r.status, r.first_bad, r.n_acks, r.n_skipped, r.n_done, r.n_batches, r.n_bytes), name
            ok = r.status == L.DV_OK
            same_or_fill(name + " out", out, h_out, r.n_bytes if ok else 0, 0xFF)
            same_or_fill(name + " batch_off", boff, h_off, r.n_batches + 1 if ok else 0, 0xFF)
            same_or_fill(name + " wait_acks", d_wa, h_wa, n, 0xFF)


def test_a_ycsb_cfg_gives_what_it_gave_beside_a_tpcc_one(eng):
    """the two workloads in turn on one context: the workspace is shared and laid out again per call"""
    import test_wire_sequence_gpu as G
    _, y_mbufs, y_e, y_k = next(c for c in S.sequence_cases() if c[0] == "mixed_cuts")
    _, t_mbufs, t_e, t_k = next(c for c in CASES if c[0] == "mixed_cuts")
    for _ in range(2):
        G.sequence_and_check(eng, y_mbufs, y_e, y_k)
        sequence_and_check(eng, t_mbufs, t_e, t_k, fills=(0xFF,))
    _, y_mbufs, y_e, y_k = next(c for c in S.sequence_cases() if c[0] == "nodes64")
    sequence_and_check(eng, t_mbufs, t_e, t_k, fills=(0x00,))
    G.sequence_and_check(eng, y_mbufs, y_e, y_k)
