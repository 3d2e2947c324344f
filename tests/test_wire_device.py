"""dv_wire_ingest_device / dv_wire_reply_fields_device on the GPU against the
host decoder (dv_wire_open / dv_wire_decode_batches through WireIngress) and
the oracle -- never against the device path itself.  The cases and what the
host decoder makes of them: tests/test_wire_device_cases.py.

The kernels' tiles (dvcc_internal.h): W = 4 batches per workgroup of
k_wire_check / k_wire_emit (kWireWave), S = 3,072 batches per scan chunk
(kWireChunk), 256 txns per tile of the reply compaction (kReplyTile).
"""
import ctypes

import numpy as np
import pytest

import _oracle as O
import wire_fmt as W
import test_wire_device_cases as C

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc.wire import DeviceWireIngress, WireIngress  # noqa: E402

ORACLE_CC = {dvcc.NO_WAIT: O.NO_WAIT, dvcc.WAIT_DIE: O.WAIT_DIE, dvcc.OCC: O.OCC}
WAVE, CHUNK, REPLY_TILE = 4, 3072, 256
GUARD = 0xA5
PAD = 64  # guard elements behind every output's capacity


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

    def __init__(self, max_txn, max_acc, forms="both"):
        g = lambda n, dt: torch.full((n * torch.empty(0, dtype=dt).element_size(),), GUARD, dtype=torch.uint8,  # noqa
                                     device="cuda").view(dt)
        T, A = max_txn + PAD, max(1, max_acc) + PAD
        self.max_txn, self.max_acc = max_txn, max_acc
        self.t = dict(txn_begin=g(T + 1, torch.int32), n_acc_dev=g(1 + PAD, torch.int32), owner=g(A, torch.uint8),
                      txn_id=g(T, torch.int64), client_startts=g(T, torch.int64), return_node=g(T, torch.int32))
        if forms in ("both", "recs"):
            self.t["recs32"] = g(A, torch.int32)
        if forms in ("both", "keys"):
            self.t.update(keys=g(A, torch.int64), types=g(A, torch.uint8), acc_txn=g(A, torch.int32))

    def struct(self):
        p = lambda k: self.t[k].data_ptr() if k in self.t else None  # noqa: E731
        return L.WireDevOut(self.max_txn, 0, self.max_acc, p("txn_begin"), p("n_acc_dev"), p("recs32"), p("keys"),
                            p("types"), p("acc_txn"), p("owner"), p("txn_id"), p("client_startts"), p("return_node"))

    def host(self):
        torch.cuda.synchronize()  # (the outputs are written on the engine's stream)
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def ingest(eng, d_buf, n_bytes, d_off, n_batches, first, outs, next_txn=0, max_req=0):
    cfg = L.WireCfg(L.YCSB, 0, C.NODE, C.NODE_CNT, C.PART_CNT, max_req, C.ROWS, None)
    out, res = outs.struct(), L.WireDevResult()
    eng._after_torch()
    rc = L.lib().dv_wire_ingest_device(eng._ctx, ctypes.byref(cfg), d_buf.data_ptr(), n_bytes, d_off.data_ptr(),
                                       n_batches, first, ctypes.byref(out), next_txn, ctypes.byref(res))
    assert rc == res.status
    return res


def upload(buf, off, shift=0):
    """the stream `shift` bytes into its tensor"""
    t = torch.zeros(shift + len(buf) + 16, dtype=torch.uint8, device="cuda")
    t[shift:shift + len(buf)] = torch.from_numpy(buf)
    return t[shift:], torch.from_numpy(off.view(np.int64)).cuda()


def check_against_host(h, res, ref, outs):
    """every output of the device call equals the host decoder's epoch `ref`
    and the guards behind n_txn / n_acc stand"""
    n, a = ref.n_txn, ref.n_acc
    assert (res.n_txn, res.n_acc) == (n, a)
    assert res.max_txn_acc == ref.max_txn_acc()
    u = lambda x, dt: x.view(dt)  # noqa: E731
    assert (u(h["txn_begin"], np.uint32)[:n + 1] == ref.txn_begin).all()
    assert u(h["n_acc_dev"], np.uint32)[0] == a
    assert (u(h["txn_id"], np.uint64)[:n] == ref.txn_id).all()
    assert (u(h["client_startts"], np.uint64)[:n] == ref.client_startts).all()
    assert (u(h["return_node"], np.uint32)[:n] == ref.return_node).all()
    assert (h["owner"][:a] == ref.owner).all()
    if "recs32" in h:
        assert (u(h["recs32"], np.uint32)[:a] == ref.to_row_records()).all()
    if "keys" in h:
        assert (u(h["keys"], np.uint64)[:a] == ref.keys).all()
        assert (h["types"][:a] == ref.types).all()
        assert (u(h["acc_txn"], np.uint32)[:a] == ref.acc_txn()).all()
    per_txn = {"txn_id", "client_startts", "return_node"}
    for k, v in h.items():
        keep = n + 1 if k == "txn_begin" else 1 if k == "n_acc_dev" else n if k in per_txn else a
        assert (v[keep:].view(np.uint8) == GUARD).all(), f"{k}: written past {keep}"


def run_and_check(eng, batches, first=0, max_txn=4096, max_acc=1 << 16, forms="both", shift=0, off=None,
                  expect=None, next_txn=0, max_req=0, buf_len=None):
    """One call over `batches`; the taken ones compared with the host decoder.
    expect: (status, n_taken) or None for (DV_OK, all)."""
    buf, off0 = C.stream(batches)
    off = off0 if off is None else off
    d_buf, d_off = upload(buf, off, shift)
    outs = Outputs(max_txn, max_acc, forms)
    res = ingest(eng, d_buf, len(buf) if buf_len is None else buf_len, d_off, len(batches), first, outs, next_txn,
                 max_req)
    status, n_taken = expect if expect is not None else (L.DV_OK, len(batches))
    assert (res.status, res.n_taken) == (status, n_taken)
    ref = C.host_decode(buf, off, first, n_taken, next_txn, max_req)
    assert res.next_txn == next_txn + ref.n_txn
    check_against_host(outs.host(), res, ref, outs)
    return res, ref


def test_every_message_shape_in_one_stream(eng):
    cases = C.good_cases()
    batches = [c[1] for c in cases]
    assert max(len(b) for b in batches) == 4096
    res, ref = run_and_check(eng, batches, next_txn=12345)
    assert ref.n_txn == sum(c[2] for c in cases) and ref.n_acc == sum(c[3] for c in cases)
    assert res.max_txn_acc == 128
    for forms in ("recs", "keys"):
        run_and_check(eng, batches, forms=forms)


@pytest.mark.parametrize("shift", [0, 1, 2, 3, 15])
def test_any_byte_alignment_of_the_buffer(eng, shift):
    run_and_check(eng, [c[1] for c in C.good_cases()], shift=shift)


@pytest.mark.parametrize("n", [1, WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_batch_counts_around_the_kernels_tiles(eng, n):
    rng = np.random.default_rng(n)
    batches = [C.small_batch(rng, src=5 + i % 3, n=i % 4, cst=i) for i in range(n)]
    run_and_check(eng, batches, max_txn=2 * CHUNK + 8, max_acc=8 * CHUNK)


def _capacity_stream():
    """26 batches of 1, 2, 3, 1, ... messages of 0..5 requests (1, 3, 12, 1, ...
    a batch) and their running counts"""
    rng = np.random.default_rng(21)
    batches, txns, accs = [], [], []
    for i in range(26):
        lens = [(2 * i + 3 * j + 1) % 6 for j in range(1 + i % 3)]
        batches.append(C.batch([C.message(C._reqs(rng, n), [0], 100 * i + j, rng) for j, n in enumerate(lens)],
                               src=5 + i % 2))
        txns.append(len(lens))
        accs.append(sum(lens))
    return batches, np.cumsum(txns), np.cumsum(accs)


def _largest_fit(ct, ca, first, max_txn, max_acc):
    """the largest batch count from `first` whose totals fit (from the case builder's counts)"""
    t0, a0 = (ct[first - 1], ca[first - 1]) if first else (0, 0)
    k = first
    while k < len(ct) and ct[k] - t0 <= max_txn and ca[k] - a0 <= max_acc:
        k += 1
    return k


@pytest.mark.parametrize("kind", ["txn_at_batch_end", "txn_one_short", "acc_cuts_first"])
def test_capacity_cuts_at_whole_batches_and_continues(eng, kind):
    batches, ct, ca = _capacity_stream()
    if kind == "txn_at_batch_end":
        max_txn, max_acc = int(ct[9]), 1 << 12
    elif kind == "txn_one_short":
        assert ct[9] - ct[8] >= 2 or ct[10] - ct[9] >= 2
        j = 9 if ct[9] - ct[8] >= 2 else 10
        max_txn, max_acc = int(ct[j]) - 1, 1 << 12
    else:
        max_txn, max_acc = int(ct[20]), int(ca[7]) + 1
        assert ca[8] - ca[7] >= 2
    first, next_txn, epochs = 0, 1000, []
    while True:
        k = _largest_fit(ct, ca, first, max_txn, max_acc)
        assert k > first
        done = k == len(batches)
        res, ref = run_and_check(eng, batches, first=first, max_txn=max_txn, max_acc=max_acc, next_txn=next_txn,
                                 expect=(L.DV_OK if done else L.WIRE_MORE, k))
        if kind == "acc_cuts_first" and not epochs:
            assert ref.n_txn < max_txn and ref.n_acc <= max_acc < ca[k]
        if kind == "txn_at_batch_end" and not epochs:
            assert ref.n_txn == max_txn
        epochs.append(ref)
        first, next_txn = k, res.next_txn
        if done:
            break
    assert len(epochs) >= 2
    # both (all) epochs together are the host decoding of the whole stream, txn ids included
    buf, off = C.stream(batches)
    whole = C.host_decode(buf, off, 0, len(batches), 1000)
    assert (np.concatenate([e.keys for e in epochs]) == whole.keys).all()
    assert (np.concatenate([e.types for e in epochs]) == whole.types).all()
    assert (np.concatenate([e.txn_id for e in epochs]) == whole.txn_id).all()
    assert (np.concatenate([e.client_startts for e in epochs]) == whole.client_startts).all()
    assert sum(e.n_txn for e in epochs) == whole.n_txn


def test_a_first_batch_that_cannot_fit(eng):
    batches, ct, ca = _capacity_stream()
    for first in (0, 5):
        t = int(ct[first] - (ct[first - 1] if first else 0))
        a = int(ca[first] - (ca[first - 1] if first else 0))
        assert t >= 2 or first == 0
        if t >= 2:
            run_and_check(eng, batches, first=first, max_txn=t - 1, expect=(L.DV_ERR_ARG, first))
        if a >= 1:
            run_and_check(eng, batches, first=first, max_acc=a - 1, expect=(L.DV_ERR_ARG, first))


def _good_row(rng, n):
    return [C.small_batch(rng, src=5 + i % 2, n=1 + i % 5, cst=10 * i) for i in range(n)]


@pytest.mark.parametrize("case", C.malformed_cases(), ids=lambda c: c[0])
def test_a_malformed_batch_stops_the_call_at_it(eng, case):
    name, bad, max_req = case
    rng = np.random.default_rng(5)
    for k in (0, 4, 8):
        batches = _good_row(rng, 9)
        batches[k] = bad
        run_and_check(eng, batches, expect=(L.DV_ERR_ARG, k), max_req=max_req, next_txn=7)


@pytest.mark.parametrize("case", C.OFF_CASES)
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
    # an end inside the allocation but past buf_len
    batches = _good_row(rng, 3)
    buf, off = C.stream(batches)
    run_and_check(eng, batches, buf_len=len(buf) - 1, expect=(L.DV_ERR_ARG, 2))


def test_a_malformed_batch_behind_the_capacity_cut_is_not_reported(eng):
    batches, ct, ca = _capacity_stream()
    bad = dict((c[0], c[1]) for c in C.malformed_cases())["acctype_2"]
    batches[12] = bad
    res, _ = run_and_check(eng, batches, max_txn=int(ct[9]), expect=(L.WIRE_MORE, 10))
    # ... and the next call reaches it
    run_and_check(eng, batches, first=10, max_txn=int(ct[9]), next_txn=res.next_txn, expect=(L.DV_ERR_ARG, 12))


def test_nothing_to_take_and_refused_arguments(eng):
    rng = np.random.default_rng(8)
    batches = _good_row(rng, 3)
    res, ref = run_and_check(eng, batches, first=3, expect=(L.DV_OK, 3))
    assert res.n_txn == 0 and res.n_acc == 0
    d_buf, d_off = upload(*C.stream(batches))
    for name, cfg, out in C.refused_arguments():
        r = L.WireDevResult()
        assert L.lib().dv_wire_ingest_device(eng._ctx, ctypes.byref(cfg), d_buf.data_ptr(), 64, d_off.data_ptr(), 3, 0,
                                             ctypes.byref(out), 0, ctypes.byref(r)) == L.DV_ERR_ARG, name
    outs = Outputs(16, 160)
    cfg = L.WireCfg(L.YCSB, 0, C.NODE, C.NODE_CNT, C.PART_CNT, 0, C.ROWS, None)
    o, r = outs.struct(), L.WireDevResult()
    assert L.lib().dv_wire_ingest_device(eng._ctx, ctypes.byref(cfg), d_buf.data_ptr(), 64, d_off.data_ptr(), 3, 4,
                                         ctypes.byref(o), 0, ctypes.byref(r)) == L.DV_ERR_ARG  # first_batch > n_batches
    assert all((v.view(np.uint8) == GUARD).all() for v in outs.host().values())


# ---- through the engine
def _client_streams(rows, n_per, seeds):
    """three clients' batches interleaved as they arrive, back to back"""
    g = dvcc.YCSBQueryGenerator(rows, zipf_theta=0.9)
    streams = [W.batches(0, 1 + c, W.ycsb_epoch_messages(g.gen(n_per, s), client_startts=100_000 * c + np.arange(n_per)))
               for c, s in enumerate(seeds)]
    out = []
    for i in range(max(len(s) for s in streams)):
        out += [s[i] for s in streams if i < len(s)]
    return out


@pytest.mark.parametrize("cc", [dvcc.NO_WAIT, dvcc.WAIT_DIE, dvcc.OCC])
@pytest.mark.parametrize("prefix", [None, 64], ids=["keys_form", "tb_form"])
def test_client_streams_ingested_on_the_device_and_decided(cc, prefix):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    rows = 1 << 16
    tab = O.YcsbTable(rows)
    f0 = tab.f0.copy()
    e = dvcc.CCEngine(cc, 4000, 40_000)
    try:
        e.load_ycsb_partition(rows)
        if prefix:
            e.set_prefix(prefix)
        batches = _client_streams(rows, 1500, (50, 51, 52))
        buf, off = C.stream(batches)
        ing = DeviceWireIngress(e, 4000, 40_000, node_id=0, node_cnt=1, synth_table_size=rows)
        host = WireIngress(L.YCSB, 1 << 16, 1 << 20, node_id=0, node_cnt=1, synth_table_size=rows)
        d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        first, n_epochs, total = 0, 0, 0
        while first < len(batches):
            dep, taken, status = ing.feed_buffer(d_buf, d_off, first)
            assert status == (L.DV_OK if taken == len(batches) else L.WIRE_MORE) and taken > first
            assert host.feed_buffer(buf, np.ascontiguousarray(off[first:taken + 1])) == []
            ep = host.take()
            assert (dep.n_txn, dep.n_acc) == (ep.n_txn, ep.n_acc) and ep.n_txn <= 4000
            c_ref, _, st_ref = O.epoch_run(ORACLE_CC[cc], tab.ix, f0, ep.n_txn, ep.txn_begin, ep.keys, ep.types)
            d_commit = torch.zeros(ep.n_txn, dtype=torch.uint8, device="cuda")
            st = e.run_epoch_device(dep, d_commit)
            c = d_commit.cpu().numpy()
            assert (c == c_ref).all()
            assert (st.committed, st.read_digest, st.write_cnt) == (st_ref.committed, st_ref.read_digest,
                                                                    st_ref.write_cnt)
            if prefix:  # records and boundaries alone, the tb path with n_acc_dev
                assert st.prefix_txn > 0 and ing.keys is None and dep.recs32 is ing.recs32
                assert dep.n_acc_dev is ing.n_acc_dev
            else:
                assert st.prefix_txn == 0 and dep.keys is ing.keys
            assert ing.respond(dep, d_commit) == host.respond(ep, c)
            first, n_epochs, total = taken, n_epochs + 1, total + ep.n_txn
        assert total == 4500 and n_epochs == 2
        assert (e.read_table(0, rows) == f0).all()
    finally:
        e.close()


def test_a_short_last_epoch_below_the_prefix_gets_both_forms():
    """records and boundaries alone are written only for an epoch that takes
    the tb-mode prefix path: one at or below the prefix's size is decoded
    again with keys / types / txn ids, and decides as the oracle does"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    rows = 1 << 16
    tab = O.YcsbTable(rows)
    f0 = tab.f0.copy()
    e = dvcc.CCEngine(dvcc.NO_WAIT, 4000, 40_000)
    try:
        e.load_ycsb_partition(rows)
        e.set_prefix(64)
        assert e.reads_tb_only(4000) and e.reads_tb_only(65) and not e.reads_tb_only(64)
        batches = _client_streams(rows, 20, (60, 61, 62))  # 60 txns in all
        buf, off = C.stream(batches)
        ing = DeviceWireIngress(e, 4000, 40_000, node_id=0, node_cnt=1, synth_table_size=rows)
        host = WireIngress(L.YCSB, 4000, 40_000, node_id=0, node_cnt=1, synth_table_size=rows)
        dep, taken, status = ing.feed_buffer(buf, off)
        assert host.feed_buffer(buf, off) == []
        ep = host.take()
        assert (taken, status, dep.n_txn, ep.n_txn) == (len(batches), L.DV_OK, 60, 60)
        assert dep.keys is ing.keys and ing.next_txn == 60
        torch.cuda.synchronize()
        assert (dep.keys[:ep.n_acc].cpu().numpy().view(np.uint64) == ep.keys).all()
        assert (dep.txn_id.cpu().numpy().view(np.uint64) == ep.txn_id).all()
        c_ref, _, st_ref = O.epoch_run(O.NO_WAIT, tab.ix, f0, ep.n_txn, ep.txn_begin, ep.keys, ep.types)
        d_commit = torch.zeros(ep.n_txn, dtype=torch.uint8, device="cuda")
        st = e.run_epoch_device(dep, d_commit)
        assert (d_commit.cpu().numpy() == c_ref).all() and st.read_digest == st_ref.read_digest
        assert st.prefix_txn == 0 and (e.read_table(0, rows) == f0).all()
    finally:
        e.close()


# ---- replies
def _reply_epoch(eng, n_txn):
    """n_txn single-message batches from two clients, interleaved"""
    rng = np.random.default_rng(n_txn)
    batches = [C.small_batch(rng, src=5 + (i * 7 // 3) % 2, n=2, cst=1_000_000 + 3 * i) for i in range(n_txn)]
    buf, off = C.stream(batches)
    kw = dict(node_id=C.NODE, node_cnt=C.NODE_CNT, part_cnt=C.PART_CNT, synth_table_size=C.ROWS)
    ing = DeviceWireIngress(eng, 1024, 4096, **kw)
    dep, taken, status = ing.feed_buffer(buf, off)
    assert (taken, status, dep.n_txn) == (n_txn, L.DV_OK, n_txn)
    host = WireIngress(L.YCSB, 1024, 4096, **kw)
    assert host.feed_buffer(buf, off) == []
    ep = host.take()
    assert len(set(ep.return_node.tolist())) == 2
    return ing, dep, host, ep


@pytest.mark.parametrize("n_txn", [REPLY_TILE - 1, REPLY_TILE, REPLY_TILE + 1, 3 * REPLY_TILE + 5])
def test_replies_of_the_committed_txns_equal_the_host_packer(eng, n_txn):
    ing, dep, host, ep = _reply_epoch(eng, n_txn)
    rng = np.random.default_rng(1)
    patterns = dict(none=np.zeros(n_txn, np.uint8), all=np.ones(n_txn, np.uint8),
                    alternating=(np.arange(n_txn) & 1).astype(np.uint8),
                    last=(np.arange(n_txn) == n_txn - 1).astype(np.uint8),
                    dense_random=(rng.random(n_txn) < 0.9).astype(np.uint8) * 7)
    for name, c in patterns.items():
        got = ing.respond(dep, torch.from_numpy(c).cuda())
        want = host.respond(ep, c)
        assert got == want, name
        assert sum(len(W.parse_batch(b)[2]) for b in got) == int((c != 0).sum()), name
    assert ing.respond(dep, torch.zeros(n_txn, dtype=torch.uint8, device="cuda")) == []


def test_replies_of_the_engines_own_commit_bytes():
    rows = C.ROWS
    e = dvcc.CCEngine(dvcc.NO_WAIT, 1024, 4096)
    try:
        e.load_ycsb_partition(rows)
        ing, dep, host, ep = _reply_epoch(e, 700)
        d_commit = torch.zeros(700, dtype=torch.uint8, device="cuda")
        st = e.run_epoch_device(dep, d_commit)
        c = d_commit.cpu().numpy()
        tab = O.YcsbTable(rows)
        c_ref, _, _ = O.epoch_run(O.NO_WAIT, tab.ix, tab.f0.copy(), ep.n_txn, ep.txn_begin, ep.keys, ep.types)
        assert (c == c_ref).all() and 0 < st.committed
        assert ing.respond(dep, d_commit) == host.respond(ep, c)
    finally:
        e.close()
