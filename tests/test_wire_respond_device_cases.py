"""CPU checks for dv_wire_respond_device: the cases' expected bytes are pinned
before the GPU sees them -- an independent numpy packer (tests/wire_rsp_cases.py,
from the format description) must agree with the host packer (dv_wire_respond),
the reference of the GPU tests -- and the entry refuses its bad arguments
before any device is touched."""
import ctypes

import numpy as np
import pytest

import wire_fmt as W
import wire_rsp_cases as R
from dvcc import _lib as L


@pytest.mark.parametrize("key", list(R.ALL), ids=R.IDS)
def test_numpy_packer_equals_host_packer(key):
    c = R.ALL[key]
    rc, buf, off, nb = R.host_pack(c)
    assert rc == L.DV_OK and off[0] == 0
    want = R.numpy_pack(c)
    assert R.split(buf, off, nb) == want
    n_ans = len(c.answered())
    assert sum(len(W.parse_batch(b, c.calvin)[2]) for b in want) == n_ans
    assert all(len(b) <= R.MSG_MAX for b in want)
    if n_ans == 0:
        assert nb == 0 and len(buf) == 0


def test_fields_have_eight_distinct_bytes_and_high_halves():
    v = R.field(np.arange(70_000), 1)
    b = v.view(np.uint8).reshape(-1, 8)
    assert all(len(set(row)) == 8 for row in b[:2048].tolist())
    assert (np.sort(b, axis=1)[:, 1:] != np.sort(b, axis=1)[:, :-1]).all()
    assert (v >= 1 << 32).all() and len(np.unique(v)) == len(v)


def test_case_list_covers_the_edges():
    for calvin, p in ((False, 48), (True, 46)):
        assert R.per(calvin) == p
        names = {n for n, cal in R.ALL if cal == calvin}
        assert {f"one_dest_{k}" for k in (p - 1, p, p + 1, 2 * p, 2 * p + 1)} <= names
        assert {f"tile_n{n}" for n in (0, 1, 255, 256, 257, 769)} <= names
        c = R.ALL[("commit_lanes_0_63_64_255", calvin)]
        assert sorted(set(np.flatnonzero(c.commit) % 256)) == [0, 63, 64, 255]
        c = R.ALL[("dest_0_and_255", calvin)]
        assert set(c.rnode[c.answered()].tolist()) == {0, 255}


def refused_arguments(p):
    """[(name, cfg, in, out)] the entry refuses before any launch, and the
    arguments it accepts; p: the address every pointer holds (device memory on
    the GPU; never followed where the context is null)"""
    def good(calvin=0):
        return (L.WireCfg(L.YCSB, calvin, 0, 1, 1, 0, 0, None),
                L.WireRspIn(4, 2, None, None, 0, 0, p, p, p, 7), L.WireRspOut(p, 256, p, 4, 0))

    def vary(name, calvin=0, node_cnt=1, **kw):
        cfg, rin, rout = good(calvin)
        cfg.node_cnt = node_cnt
        for k, v in kw.items():
            setattr(rin if k in dict(rin._fields_) else rout, k, v)
        return name, cfg, rin, rout

    return [vary("no txn_id", txn_id=None), vary("no return_node", return_node=None),
            vary("no client_startts outside CALVIN", client_startts=None),
            vary("commit and src", commit=p, src=p), vary("n_dest 0", n_dest=0),
            vary("n_dest above the limit", n_dest=L.WIRE_DEST_MAX + 1), vary("no out", out=None),
            vary("no batch_off", batch_off=None), vary("out not dword aligned", out=p + 2),
            vary("out byte aligned", out=p + 1), vary("zero node_cnt", node_cnt=0),
            vary("zero node_cnt under CALVIN", 1, node_cnt=0, client_startts=None)], good


def call(ctx, cfg, rin, rout, res):
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    return L.lib().dv_wire_respond_device(ctx, ref(cfg), ref(rin), ref(rout), ref(res))


def test_the_entry_refuses_its_bad_arguments_with_a_null_context():
    """DV_ERR_ARG before any device is touched, *res untouched; fails where
    the symbol is missing.  The GPU tests repeat every refusal on a live
    context, where only the named argument is at fault."""
    a = np.zeros(64, np.uint64)
    bad, good = refused_arguments(a.ctypes.data)
    cfg, rin, rout = good()
    res = L.WireRspResult(55, 66, 77, 0, 88)
    assert call(None, cfg, rin, rout, res) == L.DV_ERR_ARG
    assert call(None, None, None, None, None) == L.DV_ERR_ARG
    for name, c, i, o in bad:
        assert call(None, c, i, o, res) == L.DV_ERR_ARG, name
    assert (res.status, res.n_batches, res.n_msgs, res.n_bytes) == (55, 66, 77, 88)


def test_struct_layouts_of_the_reply_packer_match_the_header(tmp_path):
    import os
    import subprocess
    structs = {"dv_wire_rsp_in": L.WireRspIn, "dv_wire_rsp_out": L.WireRspOut, "dv_wire_rsp_result": L.WireRspResult}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dvcc.h"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in cls._fields_:
            lines.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines.append(f'printf("dest_max %d\\n", DV_WIRE_DEST_MAX);')
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
    assert int(got["dest_max"]) == L.WIRE_DEST_MAX
