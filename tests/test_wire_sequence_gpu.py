"""The CALVIN sequencer on the GPU (dv_wire_sequence_device,
dv_wire_sequence_acks_device) against the host functions (dv_wire_sequence,
dv_wire_sequence_acks), which tests/test_wire_sequence_cpu.py pins against the
independent model -- never against the device path itself.  Every output lies
in guarded device memory.  This file: the cases of the CPU suite and one batch
end to end through DeviceSequencer, a CALVIN ingest, the engine and back.
The sizes at the kernels' tiles: tests/test_wire_sequence_cases_gpu.py.
"""
import ctypes

import numpy as np
import pytest

import _oracle as O
import wire_fmt as W
import wire_seq as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc import wire as DW  # noqa: E402

GUARD, PAD = 0xA5, 64


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    e = dvcc.CCEngine(dvcc.CALVIN, 8192, 1 << 17)
    yield e
    e.close()


def guarded(n, dt, lead=0):
    """n elements of dt behind `lead` bytes, PAD elements more, every byte GUARD -> (the whole tensor, its view at lead)"""
    size = torch.empty(0, dtype=dt).element_size()
    t = torch.full((lead + (n + PAD) * size,), GUARD, dtype=torch.uint8, device="cuda")
    return t, t[lead:].view(dt)


def upload(buf, off, shift=0):
    """the queue `shift` bytes into a 16-byte aligned tensor"""
    t = torch.zeros(shift + len(buf) + 32, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[shift:shift + len(buf)] = torch.from_numpy(buf)
    return t[shift:], torch.from_numpy(off.view(np.int64)).cuda()


def cfg_of(k):
    return DW._seq_cfg(k["node_id"], k["node_cnt"], k["part_cnt"], k["table"], k["max_req"])


def host_sequence(mbufs, batch_id, k, first=0, **extra):
    buf, off = S.queue(mbufs)
    return DW.sequence_host(buf, off, batch_id, node_id=k["node_id"], node_cnt=k["node_cnt"], part_cnt=k["part_cnt"],
                            synth_table_size=k["table"], n_dest=k["n_dest"], max_txn=k["max_txn"],
                            max_req=k["max_req"], first_batch=first, **extra)


def same_or_guard(name, dev, ref, n):
    """dev (a guarded device view) holds ref[:n] and nothing behind it"""
    h = dev.cpu().numpy().view(ref.dtype)
    assert (h[:n] == ref[:n]).all(), name
    assert (h[n:].view(np.uint8) == GUARD).all(), f"{name}: written past {n}"


def sequence_and_check(eng, mbufs, batch_id, k, first=0, cap=None, max_batches=None, shift=0, out_lead=0, ref=None):
    """One device call over guarded outputs against the host function with the
    same capacities: the result record, every output, the guards.  Returns the
    host's SequencedBatch."""
    buf, off = S.queue(mbufs)
    ref = host_sequence(mbufs, batch_id, k, first, cap=cap, max_batches=max_batches) if ref is None else ref
    room = DW._seq_room(len(buf), k["node_cnt"])
    cap, max_b = room[0] if cap is None else cap, room[1] if max_batches is None else max_batches
    d_buf, d_off = upload(buf, off, shift)
    T = k["max_txn"]
    whole_out, out = guarded(max(cap, 4), torch.uint8, out_lead)
    _, boff = guarded(max_b + 1, torch.int64)
    _, dfirst = guarded(k["node_cnt"] + 1, torch.int32)
    _, wc = guarded(T, torch.int32)
    _, ws = guarded(T, torch.int64)
    _, wa = guarded(T, torch.int32)
    sin = L.WireSeqIn(d_buf.data_ptr(), len(buf), d_off.data_ptr(), len(mbufs), first, batch_id, k["n_dest"], T)
    sout = L.WireSeqOut(out.data_ptr(), cap, boff.data_ptr(), max_b, 0, dfirst.data_ptr(), wc.data_ptr(),
                        ws.data_ptr(), wa.data_ptr())
    res = L.WireSeqResult(status=77)
    cfg = cfg_of(k)
    eng._after_torch()
    rc = L.lib().dv_wire_sequence_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(sin), ctypes.byref(sout),
                                         ctypes.byref(res))
    torch.cuda.synchronize()
    r = ref.result
    got = (rc, res.status, res.n_taken, res.n_txn, res.n_out, res.n_msgs, res.n_bytes)
    assert got == (r.status, r.status, r.n_taken, r.n_txn, r.n_out, r.n_msgs, r.n_bytes), (got, r.n_bytes, r.n_out)
    refused = r.n_bytes > cap or r.n_out > max_b
    same_or_guard("out", out, ref.out, 0 if refused else r.n_bytes)
    assert (whole_out[:out_lead].cpu().numpy() == GUARD).all()
    same_or_guard("batch_off", boff, ref.batch_off, 0 if refused else r.n_out + 1)
    same_or_guard("dest_first", dfirst, ref.dest_first, 0 if refused else k["node_cnt"] + 1)
    n = 0 if refused else r.n_txn
    same_or_guard("wait_client", wc, ref.wait_client, n)
    same_or_guard("wait_startts", ws, ref.wait_startts, n)
    same_or_guard("wait_acks", wa, ref.wait_acks, n)
    return ref


def acks_and_check(eng, mbufs, batch_id, wait, k, cap=None, max_batches=None, shift=0):
    """One device call against the host function over the same wait list;
    returns (the new wait_acks, the host's result)."""
    buf, off = S.queue(mbufs)
    wc = np.array([w[0] for w in wait], np.uint32)
    ws = np.array([w[1] for w in wait], np.uint64)
    wa = np.array([w[2] for w in wait], np.uint32)
    n = len(wait)
    h_wa = wa.copy()
    h_out, h_off, r = DW.sequence_acks_host(buf, off, batch_id, wc, ws, h_wa, cap=cap, max_batches=max_batches, **k)
    room = DW._seq_rsp_room(n, k["n_dest"])
    cap, max_b = room[0] if cap is None else cap, room[1] if max_batches is None else max_batches
    d_buf, d_off = upload(buf if len(buf) else np.zeros(1, np.uint8), off, shift)
    _, out = guarded(max(cap, 4), torch.uint8)
    _, boff = guarded(max_b + 1, torch.int64)
    _, d_wa = guarded(max(n, 1), torch.int32)
    d_wa[:n] = torch.from_numpy(wa.view(np.int32))
    d_wc, d_ws = torch.from_numpy(wc.view(np.int32)).cuda(), torch.from_numpy(ws.view(np.int64)).cuda()
    ain = L.WireSeqAckIn(d_buf.data_ptr(), len(buf), d_off.data_ptr(), len(mbufs), k["n_dest"], batch_id, n, 0,
                         d_wc.data_ptr(), d_ws.data_ptr(), d_wa.data_ptr())
    rout = L.WireRspOut(out.data_ptr(), cap, boff.data_ptr(), max_b, 0)
    res = L.WireSeqAckResult(status=77)
    cfg = DW._seq_cfg(k["node_id"], k["node_cnt"], 1, 0, 0)
    eng._after_torch()
    rc = L.lib().dv_wire_sequence_acks_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(ain), ctypes.byref(rout),
                                              ctypes.byref(res))
    torch.cuda.synchronize()
    got = (rc, res.status, res.first_bad, res.n_acks, res.n_skipped, res.n_done, res.n_batches, res.n_bytes)
    assert got == (r.status, r.status, r.first_bad, r.n_acks, r.n_skipped, r.n_done, r.n_batches, r.n_bytes), got
    ok = r.status == L.DV_OK
    same_or_guard("out", out, h_out, r.n_bytes if ok else 0)
    same_or_guard("batch_off", boff, h_off, r.n_batches + 1 if ok else 0)
    same_or_guard("wait_acks", d_wa, h_wa, n)
    return h_wa, r


CASES = S.sequence_cases()


@pytest.mark.parametrize("name,mbufs,batch_id,k", CASES, ids=[c[0] for c in CASES])
def test_sequence_equals_the_host_function(eng, name, mbufs, batch_id, k):
    ref = sequence_and_check(eng, mbufs, batch_id, k)
    assert ref.result.status == L.DV_OK and ref.result.n_taken == len(mbufs)


def test_max_txn_cap_and_max_batches_at_their_edges(eng):
    by = {c[0]: c for c in CASES}
    _, mbufs, e, k = by["two_nodes"]
    n = host_sequence(mbufs, e, k).result.n_txn
    for max_txn, status in ((n, L.DV_OK), (n - 1, L.WIRE_MORE), (1, L.DV_ERR_ARG)):
        ref = sequence_and_check(eng, mbufs, e, dict(k, max_txn=max_txn))
        assert ref.result.status == status
    kk = dict(k, max_txn=n - 1)
    first = host_sequence(mbufs, e, kk).result.n_taken
    assert sequence_and_check(eng, mbufs, e + 1, kk, first=first).result.status == L.DV_OK
    _, mbufs, e, k = by["mixed_cuts"]
    free = host_sequence(mbufs, e, k).result
    assert sequence_and_check(eng, mbufs, e, k, cap=free.n_bytes, max_batches=free.n_out).result.status == L.DV_OK
    for extra in (dict(cap=free.n_bytes - 1), dict(max_batches=free.n_out - 1)):
        assert sequence_and_check(eng, mbufs, e, k, **extra).result.status == L.DV_ERR_ARG


MALFORMED = S.malformed_cases()


@pytest.mark.parametrize("name,mbufs,k,n_taken", MALFORMED, ids=[c[0] for c in MALFORMED])
def test_a_malformed_mbuf_stops_the_batch(eng, name, mbufs, k, n_taken):
    ref = sequence_and_check(eng, mbufs, 4, k)
    assert ref.result.status == L.DV_ERR_ARG and ref.result.n_taken == n_taken


ACKS = S.ack_cases()


@pytest.mark.parametrize("name,wait,batch_id,calls,k", ACKS, ids=[c[0] for c in ACKS])
def test_acks_equal_the_host_function(eng, name, wait, batch_id, calls, k):
    for mbufs in calls:
        wa, _ = acks_and_check(eng, mbufs, batch_id, wait, k)
        wait = [(c, s, int(a)) for (c, s, _), a in zip(wait, wa)]


def test_reply_capacities_refuse_the_acks_whole(eng):
    k = dict(node_id=0, node_cnt=1, n_dest=3)
    wait = [(1, 7, 1), (2, 8, 1), (1, 9, 1)]
    mbufs = [S.ack_mbuf(0, 0, [(0, 3), (1, 3), (2, 3)])]
    for extra in (dict(cap=2 * 12 + 3 * 92 - 1), dict(max_batches=1)):
        wa, r = acks_and_check(eng, mbufs, 3, wait, k, **extra)
        assert r.status == L.DV_ERR_ARG and wa.tolist() == [1, 1, 1]
    wa, r = acks_and_check(eng, mbufs, 3, wait, k, cap=2 * 12 + 3 * 92, max_batches=2)
    assert r.status == L.DV_OK and not wa.any()


def test_one_batch_end_to_end_on_one_gpu():
    """Clients' mbufs -> DeviceSequencer (node 1 of 2, part_cnt 1: every txn's
    participant is node 0) -> its stream for node 0 into a CALVIN ingest as
    node 0 -> the epoch decided and executed, compared with the oracle ->
    respond_device's acks -> DeviceSequencer.acks: one CL_RSP per txn to its
    client with its client_startts, no ack outstanding, and node 1's own
    stream the RDONE alone."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    rows, n, E = 1 << 16, 3000, 6
    g = dvcc.YCSBQueryGenerator(rows, zipf_theta=0.6, txn_write_perc=1.0, tup_write_perc=0.5)
    ep = g.gen(n, 91)
    cst = 5000 + 7 * np.arange(n)
    msgs = W.ycsb_epoch_messages(ep, client_startts=cst, batch_id=W.U64_MAX)  # (a CALVIN build's header)
    assert msgs[0] == S.client_query([(int(ep.types[i]), int(ep.keys[i])) for i in range(int(ep.txn_begin[1]))], [0],
                                     int(cst[0]))
    clients = [2, 3, 4]
    mbufs = S.clients(msgs, 1, 2, n_clients=3, per=40)
    client_of = [c for b in mbufs for c in [int.from_bytes(b[4:8], "little")] * int.from_bytes(b[8:12], "little")]
    assert set(client_of) == set(clients)
    tab = O.YcsbTable(rows)
    f0 = tab.f0.copy()
    eng = dvcc.CCEngine(dvcc.CALVIN, n, 20 * n)
    try:
        eng.load_ycsb_partition(rows)
        seq = dvcc.DeviceSequencer(eng, node_id=1, node_cnt=2, part_cnt=1, synth_table_size=rows, max_req=0, max_txn=n,
                                   n_dest=5)
        buf, off = S.queue(mbufs)
        out, boff, dfirst, res = seq.sequence(buf, off, E)
        assert (res.status, res.n_taken, res.n_txn, res.n_msgs) == (L.DV_OK, len(mbufs), n, n)
        torch.cuda.synchronize()
        first = dfirst.cpu().numpy().view(np.uint32).tolist()
        h_off = boff.cpu().numpy().view(np.uint64)
        assert first[2] == res.n_out and first[1] == res.n_out - 1
        own = out[int(h_off[first[1]]):int(h_off[first[2]])].cpu().numpy().tobytes()
        assert own == W.batches(1, 1, [W.rdone(E)])[0]  # node 1's own stream: the RDONE alone
        # node 0's stream, in device memory as it is, into node 0's ingest
        lo, hi = int(h_off[first[0]]), int(h_off[first[1]])
        s_off = torch.from_numpy((h_off[first[0]:first[1] + 1] - h_off[first[0]]).view(np.int64)).cuda()
        ing = DW.CalvinDeviceWireIngress(eng, n, 20 * n, node_id=0, node_cnt=2, part_cnt=1, synth_table_size=rows)
        dep, cursors = ing.sequence([(out[lo:hi], s_off)])
        assert (dep.n_txn, dep.n_acc, dep.rdone, dep.batch_id) == (n, ep.n_acc, 1, E)
        c_ref, g_ref, st_ref = O.epoch_run(O.CALVIN, tab.ix, f0, n, ep.txn_begin, ep.keys, ep.types, want_grant=True)
        d_commit = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_grant = torch.zeros(ep.n_acc, dtype=torch.int32, device="cuda")
        st = eng.run_epoch_device(dep, d_commit, d_grant)
        assert (d_commit.cpu().numpy() == c_ref).all()
        assert (d_grant.cpu().numpy().view(np.uint32) == g_ref).all()
        assert st.read_digest == st_ref.read_digest
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
        assert answered == {t: (client_of[t], int(cst[t])) for t in range(n)}
        assert (eng.read_table(0, rows) == f0).all()
    finally:
        eng.close()
