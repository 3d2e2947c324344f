"""dv_wire_ingest_device_tpcc on the GPU against the host decoder (dv_wire_open
/ dv_wire_decode_batches through WireIngress) and the oracle -- never against
the device path itself.  The cases and what the host decoder makes of them:
tests/test_wire_device_tpcc_cases.py.

The kernels' tiles (dvcc_internal.h): W = 4 batches per workgroup of
k_wire_check_tpcc / k_wire_emit_tpcc (kWireWave), S = 3,072 batches per scan
chunk (kWireChunk).  The decode tests run on a YCSB context: the entry takes
the stream and its per-call words from the context, the access lists from
cfg->tpcc.
"""
import ctypes
import struct

import numpy as np
import pytest

import _oracle as O
import wire_fmt as W
import test_wire_device_tpcc_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc import tpcc as T  # noqa: E402
from dvcc.engine import LoopTrack  # noqa: E402
from dvcc.wire import TpccDeviceWireIngress, WireIngress, tpcc_gen_queries  # noqa: E402

ORACLE_CC = {dvcc.NO_WAIT: O.NO_WAIT, dvcc.WAIT_DIE: O.WAIT_DIE, dvcc.OCC: O.OCC}
WAVE, CHUNK = 4, 3072
GUARD = 0xA5
PAD = 64  # guard elements behind every output's capacity
PER_TXN = {"txn_type": torch.uint8, "txn_id": torch.int64, "client_startts": torch.int64, "return_node": torch.int32}
PER_ACC = {"keys": torch.int64, "types": torch.uint8, "acc_txn": torch.int32, "tables": torch.uint8,
           "args": torch.int64, "owner": torch.uint8}


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    e = dvcc.CCEngine(dvcc.NO_WAIT, 8192, 1 << 17)
    yield e
    e.close()


class Outputs:
    """device output buffers of max_txn / max_acc, every byte GUARD, PAD more
    elements behind each"""

    def __init__(self, max_txn, max_acc):
        g = lambda n, dt: torch.full((n * torch.empty(0, dtype=dt).element_size(),), GUARD, dtype=torch.uint8,  # noqa
                                     device="cuda").view(dt)
        T_, A = max_txn + PAD, max(1, max_acc) + PAD
        self.max_txn, self.max_acc = max_txn, max_acc
        self.t = dict(txn_begin=g(T_ + 1, torch.int32), n_acc_dev=g(1 + PAD, torch.int32))
        self.t.update({k: g(T_, dt) for k, dt in PER_TXN.items()})
        self.t.update({k: g(A, dt) for k, dt in PER_ACC.items()})

    def struct(self):
        p = lambda k: self.t[k].data_ptr()  # noqa: E731
        return L.WireTpccDevOut(self.max_txn, 0, self.max_acc, p("txn_begin"), p("n_acc_dev"), p("keys"), p("types"),
                                p("acc_txn"), p("tables"), p("args"), p("txn_type"), p("owner"), p("txn_id"),
                                p("client_startts"), p("return_node"))

    def host(self):
        torch.cuda.synchronize()  # (the outputs are written on the engine's stream)
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def ingest(eng, d_buf, n_bytes, d_off, n_batches, first, outs, next_txn=0, pset="base"):
    cfg = C.wire_cfg(pset)
    out, res = outs.struct(), L.WireDevResult()
    eng._after_torch()
    rc = L.lib().dv_wire_ingest_device_tpcc(eng._ctx, ctypes.byref(cfg), d_buf.data_ptr(), n_bytes, d_off.data_ptr(),
                                            n_batches, first, ctypes.byref(out), next_txn, ctypes.byref(res))
    assert rc == res.status
    return res


def upload(buf, off, shift=0):
    """the stream `shift` bytes into its tensor"""
    t = torch.zeros(shift + len(buf) + 16, dtype=torch.uint8, device="cuda")
    t[shift:shift + len(buf)] = torch.from_numpy(buf)
    return t[shift:], torch.from_numpy(off.view(np.int64)).cuda()


def check_against_host(h, res, ref):
    """every output of the device call equals the host decoder's epoch `ref`
    and the guards behind n_txn / n_acc stand"""
    n, a = ref.n_txn, ref.n_acc
    assert (res.n_txn, res.n_acc) == (n, a)
    assert res.max_txn_acc == ref.max_txn_acc()
    u = lambda x, dt: x.view(dt)  # noqa: E731
    assert (u(h["txn_begin"], np.uint32)[:n + 1] == ref.txn_begin).all()
    assert u(h["n_acc_dev"], np.uint32)[0] == a
    assert (h["txn_type"][:n] == ref.txn_type).all()
    assert (u(h["txn_id"], np.uint64)[:n] == ref.txn_id).all()
    assert (u(h["client_startts"], np.uint64)[:n] == ref.client_startts).all()
    assert (u(h["return_node"], np.uint32)[:n] == ref.return_node).all()
    for k, dt in (("keys", np.uint64), ("args", np.uint64)):
        d = np.flatnonzero(u(h[k], dt)[:a] != getattr(ref, k))
        assert d.size == 0, f"{k} at {d[:5]}: {u(h[k], dt)[d[:5]]} for {getattr(ref, k)[d[:5]]}"
    assert (h["types"][:a] == ref.types).all()
    assert (h["tables"][:a] == ref.tables).all()
    assert (h["owner"][:a] == ref.owner).all()
    assert (u(h["acc_txn"], np.uint32)[:a] == ref.acc_txn()).all()
    for k, v in h.items():
        keep = n + 1 if k == "txn_begin" else 1 if k == "n_acc_dev" else n if k in PER_TXN else a
        assert (v[keep:].view(np.uint8) == GUARD).all(), f"{k}: written past {keep}"


def run_and_check(eng, batches, first=0, max_txn=4096, max_acc=1 << 16, shift=0, off=None, expect=None, next_txn=0,
                  pset="base", buf_len=None):
    """One call over `batches`; the taken ones compared with the host decoder.
    expect: (status, n_taken) or None for (DV_OK, all)."""
    buf, off0 = C.stream(batches)
    off = off0 if off is None else off
    d_buf, d_off = upload(buf, off, shift)
    outs = Outputs(max_txn, max_acc)
    res = ingest(eng, d_buf, len(buf) if buf_len is None else buf_len, d_off, len(batches), first, outs, next_txn, pset)
    status, n_taken = expect if expect is not None else (L.DV_OK, len(batches))
    assert (res.status, res.n_taken) == (status, n_taken)
    ref = C.host_decode(buf, off, first, n_taken, next_txn, pset)
    assert res.next_txn == next_txn + ref.n_txn
    check_against_host(outs.host(), res, ref)
    return res, ref


@pytest.mark.parametrize("pset", list(C.PSETS))
def test_every_message_shape_in_one_stream(eng, pset):
    cases = C.good_cases(pset)
    batches = [c[1] for c in cases]
    assert max(len(b) for b in batches) == 4096
    res, ref = run_and_check(eng, batches, next_txn=12345, pset=pset)
    assert ref.n_txn == sum(c[2] for c in cases) and ref.n_acc == sum(c[3] for c in cases)
    assert res.max_txn_acc == 127 and set(ref.tables.tolist()) == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("shift", [0, 1, 3, 15])
def test_any_byte_alignment_of_the_buffer(eng, shift):
    run_and_check(eng, [c[1] for c in C.good_cases()], shift=shift)


@pytest.mark.parametrize("n", [1, WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_batch_counts_around_the_kernels_tiles(eng, n):
    rng = np.random.default_rng(n)
    batches = [C.small_batch(rng, src=5 + i % 3, cst=i, kind=i % 2) for i in range(n)]  # one Payment a batch
    run_and_check(eng, batches, max_txn=CHUNK + 8, max_acc=3 * CHUNK + 64)


def _capacity_stream():
    """14 batches of 1, 2, 3, 1, ... small messages, batch 6 one NewOrder of 62
    items (127 accesses), and their running counts"""
    rng = np.random.default_rng(21)
    p = C.PSETS["base"]
    batches, txns, accs = [], [], []
    for i in range(14):
        if i == 6:
            qs = [C.neworder(C._items(rng, 62, p, 1))]
        else:
            qs = [[C.pay(1, 1 + j, 1 + i), C.neworder(C._items(rng, 1 + (i + j) % 4, p, 1)),
                   C.pay(2, 2, 0, name=b"CALLY")][(i + j) % 3] for j in range(1 + i % 3)]
        batches.append(C.batch([C.tmsg(q, 100 * i + j) for j, q in enumerate(qs)], src=5 + i % 2))
        txns.append(len(qs))
        accs.append(sum(C._acc(q) for q in qs))
    return batches, np.cumsum(txns), np.cumsum(accs)


def _largest_fit(ct, ca, first, max_txn, max_acc):
    """the largest batch count from `first` whose totals fit (from the case builder's counts)"""
    t0, a0 = (ct[first - 1], ca[first - 1]) if first else (0, 0)
    k = first
    while k < len(ct) and ct[k] - t0 <= max_txn and ca[k] - a0 <= max_acc:
        k += 1
    return k


@pytest.mark.parametrize("kind", ["txn_at_batch_end", "txn_one_short", "acc_inside_the_long_neworder"])
def test_capacity_cuts_at_whole_batches_and_continues(eng, kind):
    batches, ct, ca = _capacity_stream()
    if kind == "txn_at_batch_end":
        max_txn, max_acc = int(ct[4]), 1 << 12
    elif kind == "txn_one_short":
        assert ct[5] - ct[4] >= 2
        max_txn, max_acc = int(ct[5]) - 1, 1 << 12
    else:  # the 127-access NewOrder straddles max_acc: its whole batch waits for the next call
        max_txn, max_acc = int(ct[13]), int(ca[5]) + 100
        assert ca[5] < max_acc < ca[6] and ca[6] - ca[5] == 127 <= max_acc
    first, next_txn, epochs = 0, 1000, []
    while True:
        k = _largest_fit(ct, ca, first, max_txn, max_acc)
        assert k > first
        done = k == len(batches)
        res, ref = run_and_check(eng, batches, first=first, max_txn=max_txn, max_acc=max_acc, next_txn=next_txn,
                                 expect=(L.DV_OK if done else L.WIRE_MORE, k))
        if kind == "acc_inside_the_long_neworder" and not epochs:
            assert k == 6 and ref.n_txn < max_txn and ref.n_acc <= max_acc
        if kind == "txn_at_batch_end" and not epochs:
            assert ref.n_txn == max_txn
        epochs.append(ref)
        first, next_txn = k, res.next_txn
        if done:
            break
    assert len(epochs) >= 2
    # all epochs together are the host decoding of the whole stream, txn ids included
    buf, off = C.stream(batches)
    whole = C.host_decode(buf, off, 0, len(batches), 1000)
    for f in ("keys", "types", "tables", "args", "txn_id", "client_startts", "txn_type"):
        assert (np.concatenate([getattr(e, f) for e in epochs]) == getattr(whole, f)).all(), f
    assert sum(e.n_txn for e in epochs) == whole.n_txn


def test_a_first_batch_that_cannot_fit(eng):
    batches, ct, ca = _capacity_stream()
    run_and_check(eng, batches, first=6, max_acc=126, expect=(L.DV_ERR_ARG, 6))
    run_and_check(eng, batches, first=6, max_acc=127, max_txn=1, expect=(L.WIRE_MORE, 7))
    for first in (0, 5):
        t = int(ct[first] - (ct[first - 1] if first else 0))
        a = int(ca[first] - (ca[first - 1] if first else 0))
        assert t >= 2 or first == 0
        if t >= 2:
            run_and_check(eng, batches, first=first, max_txn=t - 1, expect=(L.DV_ERR_ARG, first))
        run_and_check(eng, batches, first=first, max_acc=a - 1, expect=(L.DV_ERR_ARG, first))


def _good_row(rng, n):
    return [C.small_batch(rng, src=5 + i % 2, cst=10 * i) for i in range(n)]


@pytest.mark.parametrize("case", C.malformed_cases(), ids=lambda c: c[0])
def test_a_malformed_batch_stops_the_call_at_it(eng, case):
    name, bad = case
    rng = np.random.default_rng(5)
    for k in (0, 4, 8):
        batches = _good_row(rng, 9)
        batches[k] = bad
        run_and_check(eng, batches, expect=(L.DV_ERR_ARG, k), next_txn=7)


@pytest.mark.parametrize("case", ["off_decreases", "off_past_buf_len"])
def test_a_bad_offset_stops_the_call_at_its_batch(eng, case):
    rng = np.random.default_rng(6)
    for k in (0, 4, 8):
        batches = _good_row(rng, 9)
        buf, off = C.stream(batches)
        if case == "off_decreases":
            if k:
                off[k + 1] = int(off[k]) - 1
            else:  # (batch 0 starts at 0: it starts at 1 and ends at 0 instead)
                off[0], off[1] = 1, 0
        else:
            off[k + 1:] = len(buf) + 8
        run_and_check(eng, batches, off=off, expect=(L.DV_ERR_ARG, k))
    batches = _good_row(rng, 3)
    buf, off = C.stream(batches)
    run_and_check(eng, batches, buf_len=len(buf) - 1, expect=(L.DV_ERR_ARG, 2))


def test_a_malformed_batch_behind_the_capacity_cut_is_not_reported(eng):
    batches, ct, ca = _capacity_stream()
    bad = dict(C.malformed_cases())["item_ol_quantity_2_56_middle"]
    batches[9] = bad
    res, _ = run_and_check(eng, batches, max_txn=int(ct[4]), expect=(L.WIRE_MORE, 5))
    # ... and a later call reaches it
    res, _ = run_and_check(eng, batches, first=5, max_txn=int(ct[8] - ct[4]), max_acc=1 << 12, next_txn=res.next_txn,
                           expect=(L.DV_ERR_ARG, 9))


def test_nothing_to_take_and_refused_arguments(eng):
    rng = np.random.default_rng(8)
    batches = _good_row(rng, 3)
    res, ref = run_and_check(eng, batches, first=3, expect=(L.DV_OK, 3))
    assert res.n_txn == 0 and res.n_acc == 0
    d_buf, d_off = upload(*C.stream(batches))
    names = set()
    for name, cfg, out in C.refused_arguments():
        names.add(name)
        assert C._ingest(eng._ctx, cfg, out, d_buf.data_ptr(), d_off.data_ptr(), n_batches=3) == L.DV_ERR_ARG, name
    assert names >= {"calvin", "ycsb", "max_txn_above_the_cap", "no_args", "no_params"}
    outs = Outputs(16, 160)
    o = outs.struct()
    assert C._ingest(eng._ctx, C.wire_cfg(), o, d_buf.data_ptr(), d_off.data_ptr(), n_batches=3,
                     first=4) == L.DV_ERR_ARG  # first_batch > n_batches
    o.max_txn = C.MAX_TXN_CAP + 1
    assert C._ingest(eng._ctx, C.wire_cfg(), o, d_buf.data_ptr(), d_off.data_ptr(), n_batches=3) == L.DV_ERR_ARG
    assert all((v.view(np.uint8) == GUARD).all() for v in outs.host().values())
    # the YCSB entry goes on refusing TPC-C
    y = L.WireDevOut(16, 0, 160, o.txn_begin, o.n_acc_dev, None, o.keys, o.types, o.acc_txn, None, None, None, None)
    r = L.WireDevResult()
    cfg = C.wire_cfg()
    assert L.lib().dv_wire_ingest_device(eng._ctx, ctypes.byref(cfg), d_buf.data_ptr(), 64, d_off.data_ptr(), 3, 0,
                                         ctypes.byref(y), 0, ctypes.byref(r)) == L.DV_ERR_ARG
    assert all((v.view(np.uint8) == GUARD).all() for v in outs.host().values())


# ---- through the engine
def _query_messages(qs, n, cst0=0):
    """tpcc_gen_queries' queries as the clients' CL_QRY messages"""
    msgs = []
    for i in range(n):
        x = qs[i]
        msgs.append(W.tpcc_query(dict(
            txn_type=x.txn_type, w_id=x.w_id, d_id=x.d_id, c_id=x.c_id, d_w_id=x.d_w_id, c_w_id=x.c_w_id,
            c_d_id=x.c_d_id, c_last=bytes(x.c_last), h_amount=x.h_amount, by_last_name=x.by_last_name,
            ol_cnt=x.ol_cnt, o_entry_d=x.o_entry_d, parts=[x.parts[k] for k in range(x.n_parts)],
            items=[(x.items[k].ol_i_id, x.items[k].ol_supply_w_id, x.items[k].ol_quantity)
                   for k in range(x.ol_cnt)]), client_startts=cst0 + i))
    return msgs


_E2E = {}


def _e2e():
    """the 3,000 queries of the host test (tests/test_wire_gpu.py), their
    stream and the epoch they expand to -- built once"""
    if not _E2E:
        pp = T.tpcc_params(num_wh=4, cust_per_dist=1000, max_items=2000)
        batches = W.batches(0, 1, _query_messages(tpcc_gen_queries(pp, 3000, 17), 3000))
        _E2E.update(pp=pp, po=O.tpcc_params(num_wh=4, cust_per_dist=1000, max_items=2000), stream=C.stream(batches),
                    n_batches=len(batches), ref=T.gen(pp, 3000, 17))
    return _E2E


@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC])
def test_tpcc_client_batches_ingested_on_the_device_and_decided(cc):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    d = _e2e()
    pp, ref = d["pp"], d["ref"]
    db = O.TpccDB(d["po"], 5)
    e = T.TpccEngine(cc, pp, 3000, seed=5)
    try:
        ing = TpccDeviceWireIngress(e, pp, 3000, 3000 * 33)
        dep, taken, status = ing.feed_buffer(*d["stream"])
        assert (taken, status, dep.n_txn, dep.n_acc) == (d["n_batches"], L.DV_OK, 3000, ref.n_acc)
        assert ing.next_txn == 3000 and dep.max_txn_acc == ref.max_txn_acc()
        torch.cuda.synchronize()
        h = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
        assert (h(dep.keys, np.uint64) == ref.keys).all() and (h(dep.args, np.uint64) == ref.args).all()
        assert (h(dep.types, np.uint8) == ref.types).all() and (h(dep.tables, np.uint8) == ref.tables).all()
        assert (h(dep.txn_begin, np.uint32) == ref.txn_begin).all()
        assert (h(dep.txn_type, np.uint8) == ref.txn_type).all() and (h(dep.owner, np.uint8) == ref.owner).all()
        assert (h(dep.acc_txn, np.uint32) == ref.acc_txn()).all()
        c_ref, o_ref, st_ref = db.epoch(ORACLE_CC[cc], ref.keys, ref.types, ref.tables, ref.args, ref.txn_begin)
        d_commit = torch.zeros(3000, dtype=torch.uint8, device="cuda")
        d_oid = torch.zeros(3000, dtype=torch.int64, device="cuda")
        st = e.run_tpcc_epoch_device(dep, dep.args, d_commit, d_oid)
        c = d_commit.cpu().numpy()
        assert (c == c_ref).all()
        assert (d_oid.cpu().numpy().view(np.uint64) == o_ref).all()
        assert st.committed == st_ref.committed and 0 < st.committed < 3000
        replies = [m for b in ing.respond(dep, d_commit) for m in W.parse_batch(b)[2]]
        assert sorted(m["client_startts"] for m in replies) == np.flatnonzero(c).tolist()
    finally:
        e.close()


def _reply_batches(node_id, txn_id, client_startts, return_node):
    """wire_fmt's encoding of the CL_RSP batches for these txns, in this
    order: one run of batches per destination, destinations ascending"""
    out = []
    for dest in sorted(set(int(r) for r in return_node)):
        msgs = [W.header(W.CL_RSP, int(t)) + struct.pack("<Q", int(c))
                for t, c, r in zip(txn_id, client_startts, return_node) if int(r) == dest]
        out += W.batches(dest, node_id, msgs)
    return out


def test_the_ingested_epoch_is_the_closed_loops_pool():
    """the same tracked loop twice, each on a freshly loaded engine: over the
    host-decoded, uploaded pool, then over the pool ingested on the device"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    cc, POOL, N, E = dvcc.WAIT_DIE, 1000, 300, 6
    pp = T.tpcc_params(num_wh=4, cust_per_dist=1000, max_items=2000)
    qs = tpcc_gen_queries(pp, POOL, 910)
    clients = [W.batches(0, 1 + k, _query_messages(qs, POOL, 5000)[k::2]) for k in range(2)]
    batches = [b for pair in zip(*clients) for b in pair] + clients[0][len(clients[1]):] + clients[1][len(clients[0]):]
    buf, off = C.stream(batches)
    host = WireIngress(L.TPCC, POOL, POOL * 33, tpcc=pp)
    assert host.feed_buffer(buf, off) == []
    pool = host.take()
    assert pool.n_txn == POOL and len(set(pool.return_node.tolist())) == 2

    def loop(eng, dpool, pargs, pb):
        trk = LoopTrack(N, 2, log_cap=N * E, epoch_cap=E).attach(eng)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        sts, bufs, cursor = eng.closed_loop(dpool, pargs, pb, N, E, d_commits=commits, track=trk)
        torch.cuda.synchronize()
        return ([c.cpu().numpy() for c in commits], int(cursor.item()), [s.committed for s in sts],
                [trk.commits(i)[0] for i in range(E)], [trk.commits(i)[1].cpu().numpy() for i in range(E)])

    eng = T.TpccEngine(cc, pp, N, seed=5)
    try:
        dpool, pargs = T.device_epoch(pool)
        want = loop(eng, dpool, pargs, torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda())
    finally:
        eng.close()
    assert 0 < sum(want[2]) < N * E  # (some txns retried)
    eng = T.TpccEngine(cc, pp, N, seed=5)
    try:
        ing = TpccDeviceWireIngress(eng, pp, POOL, POOL * 33)
        dep, taken, status = ing.feed_buffer(buf, off)
        assert (taken, status, dep.n_txn, dep.n_acc) == (len(batches), L.DV_OK, POOL, pool.n_acc)
        got = loop(eng, dep, dep.args, dep.txn_begin)
        for k in range(E):
            assert (got[0][k] == want[0][k]).all(), f"epoch {k}: commit bytes"
            src = want[3][k].cpu().numpy()
            assert (got[3][k].cpu().numpy() == src).all() and (got[4][k] == want[4][k]).all(), f"epoch {k}: commit log"
            assert ing.respond_logged(got[3][k]) == _reply_batches(0, pool.txn_id[src], pool.client_startts[src],
                                                                   pool.return_node[src]), f"epoch {k}: replies"
        assert got[1] == want[1] and got[2] == want[2]
    finally:
        eng.close()
