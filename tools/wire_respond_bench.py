"""An epoch's reply mbufs (CL_RSP / CALVIN_ACK) from reply fields in device
memory, three ways on one box, alternated and best of --reps,
  (a) today's path with the Python wrapper taken out: dv_wire_reply_fields_device
      (where commit bytes select), the fields copied to pinned host arrays,
      dv_wire_respond (one core) into a preallocated buffer;
  (b) dv_wire_respond_device + the packed bytes and offsets copied to pinned
      host arrays;
  (c) dv_wire_respond_device, the bytes left resident;
each timed by the host clock around --iters calls that end in a device
synchronise, reported per call.  Then the packer's per-kernel time
(dv_kernel_times), the emit kernel's bytes written per second, and a check that
(b)'s bytes and offsets equal (a)'s.  Prints one JSON line.

Shapes (--shape):
  d       config D's epoch (1,048,576 YCSB txns, theta 0.9) with the NO_WAIT
          commit bytes of a real run, four clients
  b       config B's CALVIN batch: 65,536 acks to one sequencer
  tpcc    a 65,536-txn TPC-C epoch (32 warehouses) with the WAIT_DIE commit
          bytes of a real run, four clients
  acks1m  1,048,576 acks over four sequencers, origin-major

    python tools/wire_respond_bench.py --shape d|b|tpcc|acks1m [--reps R] [--iters K] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deneva-plus_amd"))
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=["d", "b", "tpcc", "acks1m"], required=True)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
args = ap.parse_args()

calvin = args.shape in ("b", "acks1m")
NODE = 0


def sync():
    torch.cuda.synchronize()


# ---- the shape: an engine (the context the packer is queued on), n, commit bytes, return nodes
d_commit = None
if args.shape == "d":
    rows, n = 16_777_216, 1_048_576
    gen = dvcc.YCSBQueryGenerator(rows, part_cnt=1, req_per_query=10, zipf_theta=0.9, txn_write_perc=1.0,
                                  tup_write_perc=0.5, part_per_txn=1, strict_ppt=1, mpr=-1.0)
    epoch = gen.gen(n, dvcc.epoch_seed(0, 7))
    eng = dvcc.CCEngine("NO_WAIT", n, epoch.n_acc)
    eng.load_ycsb_partition(rows)
    d_commit = torch.zeros(n, dtype=torch.uint8, device="cuda")
    eng.run_epoch_device(dvcc.DeviceEpoch(epoch), d_commit)
elif args.shape == "tpcc":
    from dvcc import tpcc as T
    n = 65_536
    pp = T.tpcc_params(32)
    epoch = T.gen(pp, n, dvcc.epoch_seed(0, 7))
    eng = T.TpccEngine(dvcc.WAIT_DIE, pp, n, seed=1)
    dep, d_args = T.device_epoch(epoch)
    d_commit = torch.zeros(n, dtype=torch.uint8, device="cuda")
    eng.run_tpcc_epoch_device(dep, d_args, d_commit, torch.zeros(n, dtype=torch.int64, device="cuda"))
else:
    n = 65_536 if args.shape == "b" else 1_048_576
    eng = dvcc.CCEngine("CALVIN", 1024, 1024)
sync()
t = np.arange(n, dtype=np.uint64)
if calvin:  # sequencers' batches concatenated origin-major
    n_seq = 1 if args.shape == "b" else 4
    rnode = (10 + t // np.uint64(n // n_seq)).astype(np.uint32)
    n_dest = 10 + n_seq
    txn_id = t * np.uint64(2)
else:  # four clients' 4 KB batches (37 queries each) as they arrive, interleaved
    rnode = (1 + (t // np.uint64(37)) % np.uint64(4)).astype(np.uint32)
    n_dest = 5
    txn_id = t + np.uint64(1 << 33)
cst = np.uint64(1_000_000) + t
d_tid, d_cst, d_rn = (torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()
                      for a in (txn_id, cst, rnode))
committed = n if d_commit is None else int(d_commit.count_nonzero().item())

msg = 88 if calvin else 84
per = (L.WIRE_MSG_MAX - L.WIRE_HDR) // msg
max_b = n // per + n_dest + 1
cap = max_b * L.WIRE_HDR + n * msg
cfg = L.WireCfg(L.YCSB, 1 if calvin else 0, NODE, 1, 1, 0, 0, None)
BATCH_ID = 4
lib = L.lib()

# (a): compacted fields on the device, pinned host arrays for them, the host packer's preallocated outputs
c_tid, c_cst, c_rn = torch.empty_like(d_tid), torch.empty_like(d_cst), torch.empty_like(d_rn)
h_tid = torch.empty(n, dtype=torch.int64).pin_memory()
h_cst = torch.empty(n, dtype=torch.int64).pin_memory()
h_rn = torch.empty(n, dtype=torch.int32).pin_memory()
a_out, a_off = np.zeros(cap, np.uint8), np.zeros(max_b + 1, np.uint64)
ones = np.ones(n, np.uint8)


def leg_a():
    if d_commit is not None:
        cnt = ctypes.c_uint32()
        L.check(lib.dv_wire_reply_fields_device(eng._ctx, d_commit.data_ptr(), n, d_tid.data_ptr(), d_cst.data_ptr(),
                                                d_rn.data_ptr(), c_tid.data_ptr(), c_cst.data_ptr(), c_rn.data_ptr(),
                                                ctypes.byref(cnt)), "dv_wire_reply_fields_device")
        c = cnt.value
        src = (c_tid, c_cst, c_rn)
    else:
        c, src = n, (d_tid, d_cst, d_rn)
    h_tid[:c].copy_(src[0][:c])
    if not calvin:
        h_cst[:c].copy_(src[1][:c])
    h_rn[:c].copy_(src[2][:c])
    sync()
    e = L.WireEpoch()
    e.n_txn = e.max_txn = c
    e.batch_id = BATCH_ID
    e.txn_id, e.return_node = h_tid.data_ptr(), h_rn.data_ptr()
    e.client_startts = None if calvin else h_cst.data_ptr()
    nb = ctypes.c_uint32()
    L.check(lib.dv_wire_respond(ctypes.byref(cfg), ctypes.byref(e), ones.ctypes.data, a_out.ctypes.data, cap,
                                a_off.ctypes.data, max_b, ctypes.byref(nb)), "dv_wire_respond")
    return nb.value


# (b), (c): the device packer's outputs, and pinned host arrays for (b)
d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
d_off = torch.empty(max_b + 1, dtype=torch.int64, device="cuda")
h_out = torch.empty(cap, dtype=torch.uint8).pin_memory()
h_off = torch.empty(max_b + 1, dtype=torch.int64).pin_memory()
rin = L.WireRspIn(n, n_dest, None if d_commit is None else d_commit.data_ptr(), None, 0, 0, d_tid.data_ptr(),
                  None if calvin else d_cst.data_ptr(), d_rn.data_ptr(), BATCH_ID)
rout = L.WireRspOut(d_out.data_ptr(), cap, d_off.data_ptr(), max_b, 0)


def pack():
    res = L.WireRspResult()
    L.check(lib.dv_wire_respond_device(eng._ctx, ctypes.byref(cfg), ctypes.byref(rin), ctypes.byref(rout),
                                       ctypes.byref(res)), "dv_wire_respond_device")
    return res


def leg_b():
    res = pack()
    sync()  # (torch's copies do not wait for the engine's stream)
    h_out[:res.n_bytes].copy_(d_out[:res.n_bytes])
    h_off[:res.n_batches + 1].copy_(d_off[:res.n_batches + 1])
    sync()
    return res


def leg_c():
    res = pack()
    sync()
    return res


def timed(leg):
    sync()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        r = leg()
    return (time.perf_counter() - t0) / args.iters, r


for leg in (leg_a, leg_b, leg_c):  # warm-up of every leg
    leg()
runs = {"a": [], "b": [], "c": []}
for _ in range(args.reps):
    for k, leg in (("a", leg_a), ("b", leg_b), ("c", leg_c)):
        dt, last = timed(leg)
        runs[k].append(dt * 1e3)
        if k == "a":
            nb_a = last
        elif k == "b":
            res_b = last

n_bytes = int(a_off[nb_a])
same = bool(res_b.n_batches == nb_a and res_b.n_bytes == n_bytes and res_b.n_msgs == committed
            and (h_out[:n_bytes].numpy() == a_out[:n_bytes]).all()
            and (h_off[:nb_a + 1].numpy().view(np.uint64) == a_off[:nb_a + 1]).all())

# per-kernel time of the resident pack
eng.set_timing(False, profile=True)
eng.kernel_times(reset=True)
for _ in range(args.reps * args.iters):
    leg_c()
kt = eng.kernel_times(reset=True)
eng.set_timing(False)
kernels_us = {k: round(ms / cnt * 1e3, 2) for k, (cnt, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])}
emit_us = kernels_us.get("k_rsp_emit_calvin" if calvin else "k_rsp_emit")

best = {k: min(v) for k, v in runs.items()}
out = {
    "shape": args.shape, "dialect": "CALVIN_ACK" if calvin else "CL_RSP", "txns": n, "answered": committed,
    "destinations": int(len(np.unique(rnode))), "reply_batches": int(nb_a), "reply_bytes": n_bytes,
    "device": torch.cuda.get_device_name(0), "reps": args.reps, "iters": args.iters,
    "a_fields_d2h_plus_host_pack_ms": best["a"], "b_device_pack_plus_d2h_ms": best["b"],
    "c_device_pack_resident_ms": best["c"], "b_over_a": best["b"] / best["a"], "c_over_a": best["c"] / best["a"],
    "c_slowest_below_a_fastest": bool(max(runs["c"]) < min(runs["a"])),
    "b_slowest_below_a_fastest": bool(max(runs["b"]) < min(runs["a"])),
    "runs_ms": {k: [round(x, 4) for x in v] for k, v in runs.items()},
    "kernels_us_per_launch": kernels_us,
    "emit_write_GBps": None if not emit_us else round(n_bytes / (emit_us * 1e-6) / 1e9, 1),
    "guide_plain_store_TBps": "6.0-6.2 (256 contiguous bytes per wave instruction)",
    "b_bytes_equal_a": same, "src_hash": L.source_hash(),
    "note": "host clock around iters calls of a leg, each ending in a device synchronise, per call; best of reps, "
            "legs alternated; device-to-host copies into pinned memory; (a) without the Python wrapper's allocations",
}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
if not same:
    sys.exit(1)
