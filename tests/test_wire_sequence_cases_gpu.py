"""dv_wire_sequence_device / dv_wire_sequence_acks_device at the sizes where
the kernels change path, against the host functions (the helpers of
tests/test_wire_sequence_gpu.py).  The tile sizes are read from the source:
kWireWave client mbufs per workgroup, kWireChunk per scan chunk, kSeqTile list
entries per workgroup of the cut search, kReplyTile replies per packer tile.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import wire_fmt as W
import wire_seq as S
import test_wire_sequence_gpu as G
from test_wire_sequence_gpu import eng  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from dvcc import _lib as L  # noqa: E402
from dvcc import wire as DW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LAYOUT = open(os.path.join(ROOT, "deneva-plus_amd", "csrc", "dvcc_wire_layout.h")).read()


def _const(name):
    m = re.search(r"constexpr\s+uint32_t\s+%s\s*=\s*([0-9* ]+);" % name, _LAYOUT)
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f)
    return v


WAVE, CHUNK, TILE, RTILE = _const("kWireWave"), _const("kWireChunk"), _const("kSeqTile"), _const("kReplyTile")
assert (WAVE, CHUNK, TILE, RTILE) == (4, 3072, 256, 256)


def test_input_at_every_byte_of_a_line_and_out_at_a_dword(eng):  # noqa: F811
    _, mbufs, e, k = next(c for c in G.CASES if c[0] == "two_nodes")
    ref = G.host_sequence(mbufs, e, k)
    for shift in range(16):
        G.sequence_and_check(eng, mbufs, e, k, shift=shift, out_lead=4 * (shift & 1), ref=ref)
    wait = [(3, 100 + t, 1) for t in range(60)]
    acks = S.ack_mbufs(1, 0, [(1 + 3 * t, 21) for t in range(60)])
    for shift in range(16):
        G.acks_and_check(eng, acks, 21, wait, dict(node_id=1, node_cnt=3, n_dest=6), shift=shift)


@pytest.mark.parametrize("nb", [WAVE - 1, WAVE, WAVE + 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_client_mbuf_counts_at_the_wave_and_the_scan_chunk(eng, nb):  # noqa: F811
    """a txn of one or two requests per client mbuf; one mbuf malformed at the end in a second call"""
    k = S.kw(node_cnt=3, part_cnt=3, max_txn=nb + 8, n_dest=6)
    mbufs = [W.batches(0, 3 + b % 3, [S.txn([b, 2 * b + 1][:1 + b % 2], 3, cst=b)])[0] for b in range(nb)]
    G.sequence_and_check(eng, mbufs, 30, k)
    G.sequence_and_check(eng, mbufs[:-1] + [mbufs[-1][:-1]], 30, k)
    G.sequence_and_check(eng, mbufs, 30, dict(k, max_txn=nb - 1))


@pytest.mark.parametrize("size", [260, 244])
@pytest.mark.parametrize("n_msgs", [TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 16])
def test_list_lengths_at_the_cut_searchs_tile(eng, n_msgs, size):  # noqa: F811
    """A destination's list (its messages and the RDONE) of TILE - 1 / TILE /
    TILE + 1 entries and around two tiles.  15 to an mbuf opens an mbuf on
    entry 255, the last of a tile; 16 to an mbuf on entry 256, the first."""
    per = (4096 - 12) // size
    assert (TILE - 1) % 15 == 0 and TILE % 16 == 0 and per == (15 if size == 260 else 16)
    k = S.kw(part_cnt=2, max_txn=3 * TILE)
    ref = G.sequence_and_check(eng, S.sized_queue(n_msgs, size), 31, k)
    assert ref.result.n_out == (n_msgs + per - 1) // per  # (a full mbuf of either size has 84 bytes left for the RDONE)


def test_a_tile_of_lone_messages_and_the_longest_jump(eng):  # noqa: F811
    """messages of half an mbuf and more (every entry opens an mbuf: the longest
    walk inside a tile) beside the smallest (the farthest next)"""
    big = [S.txn(list(range(i, i + 86)), 1, cst=i) for i in range(TILE + 40)]  # 2,180 bytes: one to an mbuf
    assert len(big[0]) > (4096 - 12) // 2
    small = [S.client_query([(0, i)], [], i) for i in range(3 * TILE)]  # 132 bytes: 30 to an mbuf
    assert len(small[0]) == 132
    k = S.kw(max_txn=4 * TILE)
    # (an mbuf each; the 84-byte RDONE still fits behind the last: 2,180 + 84 <= 4,084)
    assert G.sequence_and_check(eng, S.clients(big, 0, 1), 32, k).result.n_out == TILE + 40
    G.sequence_and_check(eng, S.clients(small, 0, 1), 32, k)
    G.sequence_and_check(eng, S.clients(big[:200] + small + big[200:], 0, 1, 3, per=5), 32, dict(k, max_txn=8 * TILE))


def test_seventy_thousand_txns_over_five_nodes(eng):  # noqa: F811
    rng = np.random.default_rng(3)
    n = 70_000
    sizes = rng.choice([1, 2, 5, 10, 16, 31], n)
    keys = rng.integers(0, 1 << 20, int(sizes.sum()))
    msgs, at = [], 0
    for t in range(n):
        r = int(sizes[t])
        ks = keys[at:at + r].tolist()
        at += r
        msgs.append(S.client_query([(i & 1, x) for i, x in enumerate(ks)], sorted({x % 10 for x in ks}), t))
    k = S.kw(node_id=3, node_cnt=5, part_cnt=10, n_dest=9, max_txn=n)
    ref = G.sequence_and_check(eng, S.clients(msgs, 3, 5, 4, per=9), 33, k)
    assert ref.result.status == L.DV_OK and ref.result.n_txn == n and ref.result.n_msgs > 2 * n


def test_completing_acks_at_the_edges_of_an_mbuf_and_of_a_reply_tile(eng):  # noqa: F811
    """Txns of two acks; the first acks come in mbufs of their own, the second
    (completing) ones fill the first and the last message of every later mbuf,
    the slots between them acks of another batch; RTILE - 1, RTILE, RTILE + 1 and
    more txns complete."""
    nid, nc, E = 2, 4, 40
    k = dict(node_id=nid, node_cnt=nc, n_dest=8)
    for n in (RTILE - 1, RTILE, RTILE + 1, 2 * RTILE + 3):
        wait = [(4 + t % 4, 900 + t, 2) for t in range(n)]
        tid = lambda t: nid + nc * t  # noqa: E731
        first = S.ack_mbufs(nid, 0, [(tid(t), E) for t in range(n)])
        second = []
        for i in range(0, n - 1, 2):  # (a completing ack first and last, 44 of batch E + 1 between them)
            second.append(S.ack_mbuf(nid, 1, [(tid(i), E)] + [(tid(0), E + 1)] * 44 + [(tid(i + 1), E)]))
        if n % 2:
            second.append(S.ack_mbuf(nid, 3, [(tid(n - 1), E)]))
        wa, r = G.acks_and_check(eng, first + second[::-1], E, wait, k)
        assert r.status == L.DV_OK and r.n_done == n and not wa.any()
        # the same acks over two calls: nothing completes in the first
        wa, r = G.acks_and_check(eng, first, E, wait, k)
        assert r.n_done == 0 and (wa == 1).all()
        wa, r = G.acks_and_check(eng, second, E, [(c, s, 1) for c, s, _ in wait], k)
        assert r.n_done == n and not wa.any()


def test_calls_refused_before_any_launch(eng):  # noqa: F811
    k = S.kw(node_id=0, node_cnt=2, part_cnt=2)
    mbufs = [W.batches(0, 2, [S.txn([1, 2], 2)])[0]]
    buf, off = S.queue(mbufs)
    d_buf, d_off = G.upload(buf, off)
    _, out = G.guarded(4096, torch.uint8)
    _, boff = G.guarded(8, torch.int64)
    _, small = G.guarded(8, torch.int32)
    _, big = G.guarded(8, torch.int64)

    def call(cfg=None, ctx=True, **ch):
        a = dict(buf=d_buf.data_ptr(), off=d_off.data_ptr(), first=0, E=5, n_dest=4, max_txn=8, out=out.data_ptr(),
                 boff=boff.data_ptr(), dfirst=small.data_ptr(), wc=small.data_ptr(), ws=big.data_ptr(),
                 wa=small.data_ptr())
        a.update(ch)
        sin = L.WireSeqIn(a["buf"], len(buf), a["off"], 1, a["first"], a["E"], a["n_dest"], a["max_txn"])
        sout = L.WireSeqOut(a["out"], 4096, a["boff"], 4, 0, a["dfirst"], a["wc"], a["ws"], a["wa"])
        res = L.WireSeqResult(status=77)
        cfg = G.cfg_of(k) if cfg is None else cfg
        rc = L.lib().dv_wire_sequence_device(eng._ctx if ctx else None, ctypes.byref(cfg), ctypes.byref(sin),
                                             ctypes.byref(sout), ctypes.byref(res))
        assert rc == L.DV_OK or res.status == 77  # (a refused call leaves the record as it was)
        return rc

    eng._after_torch()
    c = lambda **f: DW._seq_cfg(f.get("node_id", 0), f.get("node_cnt", 2), f.get("part_cnt", 2), 1 << 20, 0)  # noqa: E731
    tpcc, plain = c(), c()
    tpcc.workload, plain.calvin = L.TPCC, 0
    for refused in (dict(ctx=False), dict(cfg=tpcc), dict(cfg=plain), dict(cfg=c(node_cnt=65)), dict(cfg=c(node_id=2)),
                    dict(cfg=c(part_cnt=0)), dict(buf=None), dict(off=None), dict(out=None), dict(boff=None),
                    dict(dfirst=None), dict(wc=None), dict(ws=None), dict(wa=None), dict(E=W.U64_MAX), dict(n_dest=1),
                    dict(n_dest=257), dict(max_txn=0), dict(max_txn=(1 << 20) + 1), dict(first=2),
                    dict(out=out.data_ptr() + 2)):
        assert call(**refused) == L.DV_ERR_ARG, refused

    def ack_call(cfg=None, **ch):
        a = dict(buf=d_buf.data_ptr(), off=d_off.data_ptr(), n_dest=4, E=5, out=out.data_ptr(), boff=boff.data_ptr(),
                 wc=small.data_ptr(), ws=big.data_ptr(), wa=small.data_ptr())
        a.update(ch)
        ain = L.WireSeqAckIn(a["buf"], len(buf), a["off"], 1, a["n_dest"], a["E"], 2, 0, a["wc"], a["ws"], a["wa"])
        rout = L.WireRspOut(a["out"], 4096, a["boff"], 4, 0)
        res = L.WireSeqAckResult(status=77)
        cfg = G.cfg_of(k) if cfg is None else cfg
        rc = L.lib().dv_wire_sequence_acks_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(ain), ctypes.byref(rout),
                                                  ctypes.byref(res))
        assert rc == L.DV_OK or res.status == 77  # (a refused call leaves the record as it was)
        return rc

    for refused in (dict(cfg=tpcc), dict(cfg=plain), dict(cfg=c(node_cnt=65)), dict(cfg=c(node_id=2)), dict(buf=None),
                    dict(off=None), dict(out=None), dict(boff=None), dict(wc=None), dict(ws=None), dict(wa=None),
                    dict(E=W.U64_MAX), dict(n_dest=0), dict(n_dest=257), dict(out=out.data_ptr() + 1)):
        assert ack_call(**refused) == L.DV_ERR_ARG, refused
    torch.cuda.synchronize()
    for t in (out, boff, small, big):
        assert (t.cpu().numpy().view(np.uint8) == G.GUARD).all()
    assert call() == L.DV_OK  # (the same arguments, nothing changed: taken)
