"""A CALVIN sequencer's batch -- clients' CL_QRY mbufs stamped, fanned out per
participant node and closed with RDONEs -- three ways on one box (DESIGN.md
5d.3), alternated, best and worst of --reps:
  (a) dv_wire_sequence on one core, with the copies it needs when the receive
      queue and the outgoing mbufs live in device memory: the queue to pinned
      host memory, the packed bytes, offsets and wait list back;
  (b) dv_wire_sequence_device + its bytes and offsets copied to pinned memory;
  (c) dv_wire_sequence_device, the bytes left resident;
each timed by the host clock around --iters calls that end in a device
synchronise, reported per call.  Every run checks that (b)'s bytes, offsets and
wait list equal (a)'s.  Then the per-kernel times (dv_kernel_times) and the
emit's bytes written per second.  Prints one JSON line.

Shapes (--shape): ten-request YCSB txns, theta 0.6, from four clients
  b    config B's CALVIN batch: 65,536 txns, one node
  b4   the same over 4 nodes at part_cnt 4
  m8   1,048,576 txns over 8 nodes at part_cnt 8
With --workload tpcc: dv_tpcc_gen_queries' queries (config E's knobs, 32
warehouses, one partition per node) encoded here as the clients' CL_QRYs of a
CALVIN build (tests/wire_fmt.tpcc_query), shapes b and b4.  A TPC-C message is
3 mod 4 bytes: the emit and the marks are the byte-granular kernels
(k_seq_emit_bytes, k_seq_marks_bytes).

    python tools/wire_sequence_bench.py --shape b|b4|m8 [--workload ycsb|tpcc] [--reps R] [--iters K] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import struct
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deneva-plus_amd"))
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc import wire as DW  # noqa: E402
from dvcc.tpcc import tpcc_params  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=["b", "b4", "m8"], required=True)
ap.add_argument("--workload", choices=["ycsb", "tpcc"], default="ycsb")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
tpcc = args.workload == "tpcc"
if tpcc and args.shape == "m8":
    ap.error("--workload tpcc has the shapes b and b4")

n, nodes = {"b": (65_536, 1), "b4": (65_536, 4), "m8": (1_048_576, 8)}[args.shape]
part_cnt, rows, R, NODE, E = nodes, 16_777_216, 10, 0, 4
n_clients, n_dest = 4, nodes + 4


def sync():
    torch.cuda.synchronize()


# ---- the receive queue: the clients' mbufs of a CALVIN build (84-byte header)
def ycsb_mbufs():
    """numpy all the way"""
    gen = dvcc.YCSBQueryGenerator(rows, part_cnt=part_cnt, req_per_query=R, zipf_theta=0.6, txn_write_perc=1.0,
                                  tup_write_perc=0.5, part_per_txn=min(part_cnt, 2), strict_ppt=0, mpr=-1.0)
    ep = gen.gen(n, dvcc.epoch_seed(0, 7))
    assert (np.diff(ep.txn_begin.astype(np.int64)) == R).all()
    req = np.dtype([("acc", "<u4"), ("pad", "<u4"), ("key", "<u8"), ("val", "u1"), ("pad2", "u1", (7,))])
    # (every query names one partition here, whatever its keys: the sequencer routes by the keys, the list is only checked)
    msg = np.dtype([("rtype", "<u4"), ("txn_id", "<u8"), ("batch_id", "<u8"), ("mq", "<u8"), ("lat", "<f8", (7,)),
                    ("cst", "<u8"), ("np", "<u8"), ("part", "<u8"), ("nreq", "<u8"), ("req", req, (R,))], align=False)
    m = np.zeros(n, dtype=msg)
    m["rtype"], m["txn_id"], m["batch_id"] = L.WIRE_CL_QRY, (1 << 64) - 1, (1 << 64) - 1
    m["mq"], m["lat"] = 12345, 0.5  # (clocks the sequencer zeroes)
    m["cst"] = 1_000_000 + np.arange(n, dtype=np.uint64)
    m["np"], m["part"], m["nreq"] = 1, 0, R
    m["req"]["acc"], m["req"]["key"] = ep.types.reshape(n, R), ep.keys.reshape(n, R)
    per = (L.WIRE_MSG_MAX - L.WIRE_HDR) // msg.itemsize
    raw = m.view(np.uint8).reshape(n, msg.itemsize)
    mbufs = [struct.pack("<III", NODE, nodes + (s // per) % n_clients, min(n, s + per) - s) + raw[s:s + per].tobytes()
             for s in range(0, n, per)]
    return mbufs


def tpcc_mbufs(pp):
    """the generated queries, a message each, packed greedily per client in runs of 16"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import wire_fmt as W
    qs = DW.tpcc_gen_queries(pp, n, 7)
    msgs = []
    for i in range(n):
        x = qs[i]
        m_ = W.tpcc_query(dict(
            txn_type=x.txn_type, w_id=x.w_id, d_id=x.d_id, c_id=x.c_id, d_w_id=x.d_w_id, c_w_id=x.c_w_id,
            c_d_id=x.c_d_id, c_last=bytes(x.c_last), h_amount=x.h_amount, by_last_name=x.by_last_name,
            ol_cnt=x.ol_cnt, o_entry_d=x.o_entry_d, rbk=x.rbk, remote=x.remote,
            parts=[x.parts[j] for j in range(x.n_parts)],
            items=[(x.items[j].ol_i_id, x.items[j].ol_supply_w_id, x.items[j].ol_quantity) for j in range(x.ol_cnt)]),
            1_000_000 + i, W.U64_MAX, W.U64_MAX)
        msgs.append(m_[:20] + struct.pack("<Q", 12345) + struct.pack("<7d", *(0.5,) * 7) + m_[84:])  # (clocks to zero)
    out = []
    for s_ in range(0, n, 16):
        out += W.batches(NODE, nodes + (s_ // 16) % n_clients, msgs[s_:s_ + 16])
    return out


pp = tpcc_params(32, part_cnt=nodes) if tpcc else None
mbufs = tpcc_mbufs(pp) if tpcc else ycsb_mbufs()
off = np.zeros(len(mbufs) + 1, np.uint64)
off[1:] = np.cumsum([len(b) for b in mbufs])
buf = np.frombuffer(b"".join(mbufs), np.uint8)
in_bytes, nb_in = len(buf), len(mbufs)

eng = dvcc.CCEngine("CALVIN", 1024, 1024)
cfg = DW._seq_cfg(NODE, nodes, part_cnt, rows, 0, pp) if tpcc else DW._seq_cfg(NODE, nodes, part_cnt, rows, 0)
lib = L.lib()
d_buf = torch.from_numpy(buf.copy()).cuda()
d_off = torch.from_numpy(off.view(np.int64)).cuda()

# the sizes from one host call with room to spare; then exact capacities for every leg
probe = DW.sequence_host(buf, off, E, node_id=NODE, node_cnt=nodes, part_cnt=part_cnt, synth_table_size=rows,
                         n_dest=n_dest, max_txn=n, **(dict(params=pp) if tpcc else {})).result
assert probe.status == L.DV_OK and probe.n_txn == n
cap, max_b = probe.n_bytes, probe.n_out

h_buf = torch.empty(in_bytes, dtype=torch.uint8).pin_memory()
a_out, a_off, a_first = np.zeros(cap, np.uint8), np.zeros(max_b + 1, np.uint64), np.zeros(nodes + 1, np.uint32)
a_wc, a_ws, a_wa = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
da_out = torch.empty(cap, dtype=torch.uint8, device="cuda")  # (a)'s bytes back where the sender reads them
da_off = torch.empty(max_b + 1, dtype=torch.int64, device="cuda")
da_w = [torch.empty(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32)]
h_off = off.copy()


def leg_a():
    h_buf.copy_(d_buf)
    sync()
    sin = L.WireSeqIn(h_buf.data_ptr(), in_bytes, h_off.ctypes.data, nb_in, 0, E, n_dest, n)
    sout = L.WireSeqOut(a_out.ctypes.data, cap, a_off.ctypes.data, max_b, 0, a_first.ctypes.data, a_wc.ctypes.data,
                        a_ws.ctypes.data, a_wa.ctypes.data)
    res = L.WireSeqResult()
    L.check(lib.dv_wire_sequence(ctypes.byref(cfg), ctypes.byref(sin), ctypes.byref(sout), ctypes.byref(res)),
            "dv_wire_sequence")
    da_out.copy_(torch.from_numpy(a_out))
    da_off.copy_(torch.from_numpy(a_off.view(np.int64)))
    for d, h in zip(da_w, (a_wc.view(np.int32), a_ws.view(np.int64), a_wa.view(np.int32))):
        d.copy_(torch.from_numpy(h))
    sync()
    return res


d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
d_boff = torch.empty(max_b + 1, dtype=torch.int64, device="cuda")
d_first = torch.empty(nodes + 1, dtype=torch.int32, device="cuda")
d_wc, d_ws, d_wa = (torch.empty(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int32))
p_out = torch.empty(cap, dtype=torch.uint8).pin_memory()
p_off = torch.empty(max_b + 1, dtype=torch.int64).pin_memory()
sin_d = L.WireSeqIn(d_buf.data_ptr(), in_bytes, d_off.data_ptr(), nb_in, 0, E, n_dest, n)
sout_d = L.WireSeqOut(d_out.data_ptr(), cap, d_boff.data_ptr(), max_b, 0, d_first.data_ptr(), d_wc.data_ptr(),
                      d_ws.data_ptr(), d_wa.data_ptr())


def seq():
    res = L.WireSeqResult()
    L.check(lib.dv_wire_sequence_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(sin_d), ctypes.byref(sout_d),
                                        ctypes.byref(res)), "dv_wire_sequence_device")
    return res


def leg_b():
    res = seq()
    sync()  # (torch's copies do not wait for the engine's stream)
    p_out[:res.n_bytes].copy_(d_out[:res.n_bytes])
    p_off[:res.n_out + 1].copy_(d_boff[:res.n_out + 1])
    sync()
    return res


def leg_c():
    res = seq()
    sync()
    return res


def timed(leg):
    sync()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        r = leg()
    return (time.perf_counter() - t0) / args.iters, r


def b_equals_a(ra, rb):
    same = (ra.n_out, ra.n_bytes, ra.n_txn, ra.n_msgs) == (rb.n_out, rb.n_bytes, rb.n_txn, rb.n_msgs)
    same = same and (p_out[:ra.n_bytes].numpy() == a_out[:ra.n_bytes]).all()
    same = same and (p_off[:ra.n_out + 1].numpy().view(np.uint64) == a_off[:ra.n_out + 1]).all()
    same = same and (d_first.cpu().numpy().view(np.uint32) == a_first).all()
    for d, h in ((d_wc, a_wc), (d_ws, a_ws), (d_wa, a_wa)):
        same = same and (d.cpu().numpy().view(h.dtype) == h).all()
    return bool(same)


for leg in (leg_a, leg_b, leg_c):  # warm-up of every leg
    leg()
runs, same = {"a": [], "b": [], "c": []}, True
for _ in range(args.reps):
    for k, leg in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
        dt, last = timed(leg)
        runs[k].append(dt * 1e3)
        if k == "a":
            res_a = last
        elif k == "b":
            same = same and b_equals_a(res_a, last)
assert same, "(b)'s bytes differ from (a)'s"

# per-kernel time of the resident call
eng.set_timing(False, profile=True)
eng.kernel_times(reset=True)
for _ in range(args.reps * args.iters):
    leg_c()
kt = eng.kernel_times(reset=True)
eng.set_timing(False)
kernels_us = {k: round(ms / cnt * 1e3, 2) for k, (cnt, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])}
emit_us = kernels_us.get("k_seq_emit_bytes" if tpcc else "k_seq_emit")
cut_us = sum(kernels_us.get(k, 0) for k in ("k_seq_tiles", "k_seq_chain", "k_seq_marks_bytes" if tpcc else "k_seq_marks"))

best, worst = {k: min(v) for k, v in runs.items()}, {k: max(v) for k, v in runs.items()}
out = {
    "shape": args.shape, "workload": args.workload, "txns": n, "nodes": nodes, "part_cnt": part_cnt, "client_mbufs": nb_in, "in_bytes": in_bytes,
    "messages_out": int(res_a.n_msgs), "mbufs_out": int(res_a.n_out), "out_bytes": int(res_a.n_bytes),
    "device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters,
    "a_host_one_core_with_copies_ms": [best["a"], worst["a"]], "b_device_plus_d2h_ms": [best["b"], worst["b"]],
    "c_device_resident_ms": [best["c"], worst["c"]], "b_over_a": best["b"] / best["a"], "c_over_a": best["c"] / best["a"],
    "c_slowest_below_a_fastest": bool(worst["c"] < best["a"]), "b_slowest_below_a_fastest": bool(worst["b"] < best["a"]),
    "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()},
    "kernels_us_per_launch": kernels_us, "cut_search_us": round(cut_us, 2),
    "emit_write_GBps": None if not emit_us else round(res_a.n_bytes / (emit_us * 1e-6) / 1e9, 1),
    "reply_emit_TBps_5d2": 3.66, "b_bytes_equal_a": same, "src_hash": L.source_hash(),
    "note": "host clock around iters calls of a leg, each ending in a device synchronise, per call; best and worst of "
            "reps, legs alternated; copies through pinned memory; (a) copies the queue down and the outputs back",
}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
