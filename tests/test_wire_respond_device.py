"""dv_wire_respond_device on the GPU: the reply mbufs packed on the device
against the host packer (dv_wire_respond), bit for bit -- never against the
device path itself.  The cases and the host packer's output for each come
from tests/wire_rsp_cases.py, whose expected bytes
tests/test_wire_respond_device_cases.py pins on the CPU.  Every output has 64
guard elements (0xA5) behind it, `out` is handed in 8-byte aligned and at a
4-byte offset, and a refused call must leave every byte at the guard value."""
import numpy as np
import pytest

import _oracle as O
import wire_fmt as W
import wire_rsp_cases as R
import test_wire_device_cases as C
from test_wire_respond_device_cases import call, refused_arguments

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import dvcc  # noqa: E402
from dvcc import LoopTrack  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc.wire import (CalvinDeviceWireIngress, DeviceWireIngress, WireEpoch, WireIngress,  # noqa: E402
                       reply_batches)

GUARD, PAD = 0xA5, 64


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    e = dvcc.CCEngine(dvcc.NO_WAIT, 8192, 1 << 17)
    yield e
    e.close()


_want = {}


def want(c):
    """the host packer's output for a case: computed once, read-only afterwards"""
    if (c.name, c.calvin) not in _want:
        rc, buf, off, nb = R.host_pack(c)
        assert rc == L.DV_OK
        _want[(c.name, c.calvin)] = (buf, off, nb)
    return _want[(c.name, c.calvin)]


def _dev(a):
    """a host array's bytes on the device (eight at least, so that an empty
    array still has an address)"""
    h = np.zeros(max(a.nbytes, 8), np.uint8)
    h[:a.nbytes] = a.view(np.uint8).ravel()
    return torch.from_numpy(h).cuda()


def run(eng, c, cap, max_batches, shift=0, commit=None):
    """one call over case c into guard-filled outputs of exactly cap bytes and
    max_batches + 1 offsets (PAD guard elements behind each), out starting
    `shift` bytes into its tensor -> (rc, result, out bytes, batch_off words),
    the host copies including the guards"""
    d_out = torch.full((shift + cap + PAD,), GUARD, dtype=torch.uint8, device="cuda")
    d_off = torch.full(((max_batches + 1 + PAD) * 8,), GUARD, dtype=torch.uint8, device="cuda")
    commit = c.commit if commit is None else commit
    held = [_dev(c.txn_id), _dev(c.cst), _dev(c.rnode), None if commit is None else _dev(commit),
            None if c.src is None else _dev(c.src)]
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rin = L.WireRspIn(c.n, c.n_dest, p(held[3]), p(held[4]), c.n_src_txn, 0, p(held[0]),
                      None if c.calvin else p(held[1]), p(held[2]), c.batch_id)
    rout = L.WireRspOut(d_out.data_ptr() + shift, cap, d_off.data_ptr(), max_batches, 0)
    assert (d_out.data_ptr() + shift) % 8 == shift % 8
    res = L.WireRspResult(status=99)
    eng._after_torch()
    rc = call(eng._ctx, R.cfg_of(c), rin, rout, res)
    torch.cuda.synchronize()
    return rc, res, d_out.cpu().numpy()[shift:], d_off.cpu().numpy().view(np.uint64)


def check_ok(c, rc, res, out, off, cap, max_batches):
    buf, woff, nb = want(c)
    assert (rc, res.status) == (L.DV_OK, L.DV_OK)
    assert (res.n_batches, res.n_bytes, res.n_msgs) == (nb, len(buf), len(c.answered()))
    assert (out[:len(buf)] == buf).all(), "reply bytes"
    assert (out[len(buf):] == GUARD).all(), "written at or past out[n_bytes]"
    assert (off[:nb + 1] == woff).all() and off[0] == 0, "batch_off"
    assert (off[nb + 1:].view(np.uint8) == GUARD).all(), "written at or past batch_off[n_batches + 1]"


def check_refused(rc, res, out, off, needed=None):
    """DV_ERR_ARG from the kernels: nothing written, the needed sizes reported"""
    assert (rc, res.status) == (L.DV_ERR_ARG, L.DV_ERR_ARG)
    assert (out == GUARD).all() and (off.view(np.uint8) == GUARD).all()
    nb, n_bytes, n_msgs = needed if needed is not None else (0, 0, 0)
    assert (res.n_batches, res.n_bytes, res.n_msgs) == (nb, n_bytes, n_msgs)


@pytest.mark.parametrize("shift", [0, 4], ids=["aligned8", "aligned4"])
@pytest.mark.parametrize("key", list(R.ALL), ids=R.IDS)
def test_replies_equal_the_host_packer(eng, key, shift):
    c = R.ALL[key]
    buf, _, nb = want(c)
    cap, mb = len(buf) + 40, nb + 3
    check_ok(c, *run(eng, c, cap, mb, shift), cap, mb)


@pytest.mark.parametrize("calvin", [False, True], ids=["rsp", "ack"])
def test_capacity_exact_and_one_below(eng, calvin):
    c = R.ALL[("tile_n769", calvin)]
    buf, _, nb = want(c)
    needed = (nb, len(buf), len(c.answered()))
    assert nb >= 3
    check_ok(c, *run(eng, c, len(buf), nb, 4), len(buf), nb)
    check_refused(*run(eng, c, len(buf) - 1, nb), needed)
    check_refused(*run(eng, c, len(buf), nb - 1, 4), needed)
    check_refused(*run(eng, c, 0, 0), needed)
    # the host packer refuses the same capacities (it writes the mbufs in front: the one stated difference)
    assert R.host_pack(c, len(buf) - 1, nb)[0] == L.DV_ERR_ARG
    assert R.host_pack(c, len(buf), nb - 1)[0] == L.DV_ERR_ARG
    assert R.host_pack(c, len(buf), nb)[0] == L.DV_OK


@pytest.mark.parametrize("calvin", [False, True], ids=["rsp", "ack"])
def test_a_return_node_out_of_range(eng, calvin):
    """refused on an answered txn, accepted on an unanswered one"""
    rng = np.random.default_rng(5)
    n = 700
    commit = (rng.random(n) < 0.5).astype(np.uint8)
    commit[[300, 301]] = (1, 0)
    rnode = rng.integers(0, 3, n)
    rnode[301] = 3  # n_dest on an unanswered txn
    ok = R.Case("node_on_unanswered", calvin, 3, rnode, commit)
    buf, _, nb = want(ok)
    check_ok(ok, *run(eng, ok, len(buf) + 8, nb + 1), len(buf) + 8, nb + 1)
    rnode = rnode.copy()
    rnode[300] = 3  # and on an answered one
    bad = R.Case("node_on_answered", calvin, 3, rnode, commit)
    check_refused(*run(eng, bad, len(buf) + 8, nb + 1))
    far = R.Case("node_far_out", calvin, 3, np.where(np.arange(n) == 699, 0xFFFFFFFF, rnode % 3), None)
    check_refused(*run(eng, far, 1 << 17, 64, 4))


@pytest.mark.parametrize("calvin", [False, True], ids=["rsp", "ack"])
def test_a_list_index_out_of_range(eng, calvin):
    rng = np.random.default_rng(6)
    rnode = rng.integers(0, 4, 600)
    src = rng.integers(0, 600, 500)
    ok = R.Case("src_last", calvin, 4, rnode, src=np.r_[src, 599])
    buf, _, nb = want(ok)
    check_ok(ok, *run(eng, ok, len(buf), nb), len(buf), nb)
    bad = R.Case("src_at_n_src_txn", calvin, 4, rnode, src=np.r_[src[:257], 600, src[257:]])
    check_refused(*run(eng, bad, len(buf) + 4096, nb + 4))


def test_refused_before_any_launch_on_a_live_context(eng):
    """each bad argument alone, every pointer a device address: DV_ERR_ARG,
    *res and the outputs untouched; then the same arguments without the fault
    are taken"""
    d = torch.full((4096,), GUARD, dtype=torch.uint8, device="cuda")
    bad, good = refused_arguments(d.data_ptr())
    res = L.WireRspResult(55, 66, 77, 0, 88)
    for name, c, i, o in bad:
        assert call(eng._ctx, c, i, o, res) == L.DV_ERR_ARG, name
    cfg, rin, rout = good()
    assert call(eng._ctx, None, rin, rout, res) == L.DV_ERR_ARG
    assert call(eng._ctx, cfg, None, rout, res) == L.DV_ERR_ARG
    assert call(eng._ctx, cfg, rin, None, res) == L.DV_ERR_ARG
    assert call(eng._ctx, cfg, rin, rout, None) == L.DV_ERR_ARG
    assert (res.status, res.n_batches, res.n_msgs, res.n_bytes) == (55, 66, 77, 88)
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == GUARD).all()
    # the accepted form of the same call: 4 txns whose fields are the guard bytes, node 0xA5A5A5A5 >= n_dest
    assert call(eng._ctx, cfg, rin, rout, res) == L.DV_ERR_ARG and res.status == L.DV_ERR_ARG
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == GUARD).all()


# ---- through the ingresses
def _client_streams(rows, n_per, seeds):
    """three clients' batches interleaved as they arrive"""
    g = dvcc.YCSBQueryGenerator(rows, zipf_theta=0.9)
    streams = [W.batches(0, 1 + c, W.ycsb_epoch_messages(g.gen(n_per, s), client_startts=(7 << 40) + 100_000 * c +
                                                         np.arange(n_per)))
               for c, s in enumerate(seeds)]
    out = []
    for i in range(max(len(s) for s in streams)):
        out += [s[i] for s in streams if i < len(s)]
    return out


def test_client_epochs_answered_on_the_device():
    """ingest on the device, decide, respond_device; against WireIngress.respond
    over the host-decoded epoch; the next epoch on the same context decides as
    the oracle does (the packer's workspace does not disturb it)"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    rows = 1 << 16
    tab = O.YcsbTable(rows)
    f0 = tab.f0.copy()
    e = dvcc.CCEngine(dvcc.NO_WAIT, 2000, 20_000)
    try:
        e.load_ycsb_partition(rows)
        batches = _client_streams(rows, 1100, (50, 51, 52))
        buf, off = C.stream(batches)
        ing = DeviceWireIngress(e, 2000, 20_000, node_id=0, node_cnt=1, synth_table_size=rows)
        ing.n_dest = 4
        host = WireIngress(L.YCSB, 1 << 16, 1 << 20, node_id=0, node_cnt=1, synth_table_size=rows)
        d_buf, d_off = torch.from_numpy(buf).cuda(), torch.from_numpy(off.view(np.int64)).cuda()
        first, n_epochs, answered = 0, 0, 0
        while first < len(batches):
            dep, taken, status = ing.feed_buffer(d_buf, d_off, first)
            assert host.feed_buffer(buf, np.ascontiguousarray(off[first:taken + 1])) == []
            ep = host.take()
            c_ref, _, st_ref = O.epoch_run(O.NO_WAIT, tab.ix, f0, ep.n_txn, ep.txn_begin, ep.keys, ep.types)
            d_commit = torch.zeros(ep.n_txn, dtype=torch.uint8, device="cuda")
            st = e.run_epoch_device(dep, d_commit)
            assert (d_commit.cpu().numpy() == c_ref).all() and st.read_digest == st_ref.read_digest
            out, boff, nb = ing.respond_device(dep, d_commit)
            got = reply_batches(out, boff, nb)
            assert got == host.respond(ep, c_ref) and nb == len(got) >= 3
            msgs = [m for b in got for m in W.parse_batch(b)[2]]
            assert len(msgs) == int(c_ref.sum()) and all(m["rtype"] == W.CL_RSP for m in msgs)
            assert {W.parse_batch(b)[0] for b in got} == {1, 2, 3}
            first, n_epochs, answered = taken, n_epochs + 1, answered + len(msgs)
        assert n_epochs == 2 and answered > 0
        assert (e.read_table(0, rows) == f0).all()
    finally:
        e.close()


def test_calvin_epochs_acknowledged_on_the_device():
    """two sequencers' streams of two Calvin batches: each epoch sequenced and
    decided on the device, acknowledged by respond_device as the host packer
    acknowledges the host-decoded epoch; the second epoch after the first's
    acks decides as the oracle does"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    rows, n = 1 << 16, 1500
    g = dvcc.YCSBQueryGenerator(rows, zipf_theta=0.6, txn_write_perc=1.0, tup_write_perc=0.5)
    tab = O.YcsbTable(rows)
    f0 = tab.f0.copy()
    streams, host = [], []
    for node in range(2):
        msgs = []
        for k, bid in enumerate((4, 5)):
            ids = (9 << 36) + node + 2 * (k * n + np.arange(n))
            msgs += W.ycsb_epoch_messages(g.gen(n, 70 + 2 * node + k), batch_id=bid, txn_ids=ids,
                                          client_startts=ids * 3) + [W.rdone(bid)]
        mbufs = W.batches(0, 10 + node, msgs)
        streams.append(C.stream(mbufs))
        w = WireIngress(L.YCSB, n, 20 * n, node_id=0, node_cnt=2, synth_table_size=rows, calvin=True)
        closed = []
        for b in mbufs:
            closed += w.feed(b)
        closed.append(w.take())
        assert [(d.n_txn, d.batch_id) for d in closed] == [(n, 4), (n, 5)]
        host.append((w, closed))
    eng = dvcc.CCEngine(dvcc.CALVIN, 2 * n, 40 * n)
    try:
        eng.load_ycsb_partition(rows)
        ing = CalvinDeviceWireIngress(eng, 2 * n, 40 * n, node_id=0, node_cnt=2, synth_table_size=rows)
        ing.n_dest = 12
        d_streams = [(torch.from_numpy(b).cuda(), torch.from_numpy(o.view(np.int64)).cuda()) for b, o in streams]
        cursors = None
        for k, bid in enumerate((4, 5)):
            dep, cursors = ing.sequence(d_streams, cursors)
            parts = [host[node][1][k] for node in range(2)]
            ep = dvcc.sequence(parts)
            c_ref, _, st_ref = O.epoch_run(O.CALVIN, tab.ix, f0, ep.n_txn, ep.txn_begin, ep.keys, ep.types)
            d_commit = torch.zeros(ep.n_txn, dtype=torch.uint8, device="cuda")
            st = eng.run_epoch_device(dep, d_commit)
            assert (d_commit.cpu().numpy() == c_ref).all() and st.read_digest == st_ref.read_digest
            whole = WireEpoch(ep.keys, ep.types, ep.txn_begin, txn_id=np.concatenate([p.txn_id for p in parts]),
                              client_startts=np.concatenate([p.client_startts for p in parts]),
                              return_node=np.concatenate([p.return_node for p in parts]), batch_id=bid)
            got = reply_batches(*ing.respond_device(dep))
            assert got == host[0][0].respond(whole)
            acks = [m for b in got for m in W.parse_batch(b, calvin=True)[2]]
            assert len(acks) == 2 * n and all(m["batch_id"] == bid and m["rc"] == 0 for m in acks)
        assert (eng.read_table(0, rows) == f0).all()
    finally:
        eng.close()


def test_a_commit_logs_slices_answered_on_the_device():
    """a closed loop over a pool ingested on the device: every epoch's slice of
    the commit log through respond_logged_device equals respond_logged (a torch
    gather and the host packer) over the same slice"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    rows, N, E, n_per = 1 << 13, 1000, 4, 800
    batches = _client_streams(rows, n_per, (70, 71, 72))
    buf, off = C.stream(batches)
    eng = dvcc.CCEngine(dvcc.NO_WAIT, 4000, 40_000)
    try:
        eng.set_prefix(None)
        eng.load_ycsb_partition(rows)
        ing = DeviceWireIngress(eng, 4000, 40_000, node_id=0, node_cnt=1, synth_table_size=rows)
        ing.n_dest = 4
        dep, taken, status = ing.feed_buffer(buf, off)
        assert (taken, status, dep.n_txn) == (len(batches), L.DV_OK, 3 * n_per)
        trk = LoopTrack(N, 2, log_cap=N * E, epoch_cap=E).attach(eng)
        commits = [torch.zeros(N, dtype=torch.uint8, device="cuda") for _ in range(E)]
        eng.closed_loop(dep, ing.txn_begin, N, E, d_commits=commits, track=trk)
        total = 0
        for i in range(E):
            src = trk.commits(i)[0]
            want_b = ing.respond_logged(src)
            got = reply_batches(*ing.respond_logged_device(src))
            assert got == want_b and len(got) >= 3, i
            total += sum(len(W.parse_batch(b)[2]) for b in got)
        assert total == sum(int(trk.commits(i)[0].numel()) for i in range(E)) > 0
        out, boff, nb = ing.respond_logged_device(trk.commits(0)[0][:0])
        assert nb == 0 and out.numel() == 0 and reply_batches(out, boff, nb) == []
    finally:
        eng.close()
