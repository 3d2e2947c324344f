"""A config-E client stream from Deneva's wire format to a device-resident TPC-C
epoch, three ways on one box: --txns queries of
dv_tpcc_gen_queries at config E's one-GPU share (32 warehouses) as runcl's
client batches (TPCCClientQueryMessage CL_QRY mbufs of at most 4 KB,
tests/wire_fmt.tpcc_query), the stream repeated --repeat times back to back,
then, alternated and best of three,
  (a) host decode (dv_wire_decode_batches, one core) + T.device_epoch upload
      -- the path before the device ingress;
  (b) upload of the raw bytes + dv_wire_ingest_device_tpcc;
  (c) dv_wire_ingest_device_tpcc with the bytes already resident;
each timed by the host clock around work that ends in a device synchronise.
Then the ingest's per-kernel time (dv_kernel_times) and a check that every
array of the device epoch equals the host decoder's.  The ingest takes the
stream and its per-call words from the context and the access lists from the
parameters, so the context here holds no TPC-C tables.  Prints one JSON line.

    python tools/wire_ingest_tpcc_bench.py [--txns N] [--repeat R] [--reps K] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deneva-plus_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dvcc  # noqa: E402
import wire_fmt as W  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc import tpcc as T  # noqa: E402
from dvcc.wire import TpccDeviceWireIngress, WireIngress, tpcc_gen_queries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--txns", type=int, default=65_536)
ap.add_argument("--repeat", type=int, default=1, help="the stream this many times back to back (16: 1M queries)")
ap.add_argument("--wh", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

pp = T.tpcc_params(args.wh)
qs = tpcc_gen_queries(pp, args.txns, 7)
msgs = []
for i in range(args.txns):
    x = qs[i]
    msgs.append(W.tpcc_query(dict(
        txn_type=x.txn_type, w_id=x.w_id, d_id=x.d_id, c_id=x.c_id, d_w_id=x.d_w_id, c_w_id=x.c_w_id,
        c_d_id=x.c_d_id, c_last=bytes(x.c_last), h_amount=x.h_amount, by_last_name=x.by_last_name, ol_cnt=x.ol_cnt,
        o_entry_d=x.o_entry_d, parts=[x.parts[k] for k in range(x.n_parts)],
        items=[(x.items[k].ol_i_id, x.items[k].ol_supply_w_id, x.items[k].ol_quantity) for k in range(x.ol_cnt)]),
        client_startts=i))
del qs
batches = W.batches(0, 1, msgs)
del msgs
buf = np.frombuffer(b"".join(batches) * args.repeat, np.uint8)
off = np.zeros(len(batches) * args.repeat + 1, np.uint64)
off[1:] = np.cumsum([len(b) for b in batches] * args.repeat)
off64 = torch.from_numpy(off.view(np.int64))
n_txn = args.txns * args.repeat
max_acc = n_txn * (3 + 2 * pp.max_items_per_txn)

eng = dvcc.CCEngine("NO_WAIT", 1024, 1024)  # (the stream and the ingest's per-call words)
host = WireIngress(L.TPCC, n_txn, max_acc, tpcc=pp)
ing = TpccDeviceWireIngress(eng, pp, n_txn, max_acc)


def sync():
    torch.cuda.synchronize()


def leg_a():
    t0 = time.perf_counter()
    closed = host.feed_buffer(buf, off)
    ep = host.take()
    t1 = time.perf_counter()
    dep, d_args = T.device_epoch(ep)
    sync()
    t2 = time.perf_counter()
    assert not closed and ep.n_txn == n_txn
    return t2 - t0, t1 - t0, ep, dep, d_args


def leg_b():
    t0 = time.perf_counter()
    d_buf, d_off = torch.from_numpy(buf).to("cuda"), off64.to("cuda")
    dep, taken, status = ing.feed_buffer(d_buf, d_off)
    sync()
    dt = time.perf_counter() - t0
    assert status == L.DV_OK and taken == len(off) - 1
    return dt, dep


d_buf, d_off = torch.from_numpy(buf).to("cuda"), off64.to("cuda")


def leg_c():
    sync()
    t0 = time.perf_counter()
    dep, taken, status = ing.feed_buffer(d_buf, d_off)
    sync()
    dt = time.perf_counter() - t0
    assert status == L.DV_OK and taken == len(off) - 1
    return dt, dep


leg_a(), leg_b(), leg_c()  # warm-up of every leg
runs = {"a": [], "a_decode": [], "b": [], "c": []}
for _ in range(args.reps):
    ta, tdec, ep, _dep, _args = leg_a()
    runs["a"].append(ta)
    runs["a_decode"].append(tdec)
    runs["b"].append(leg_b()[0])
    tc, dep = leg_c()
    runs["c"].append(tc)
best = {k: min(v) for k, v in runs.items()}

# the device epoch against the host decoder's, every array
sync()
h = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
same = bool(dep.n_txn == ep.n_txn and dep.n_acc == ep.n_acc
            and (h(dep.txn_begin, np.uint32) == ep.txn_begin).all()
            and (h(dep.keys, np.uint64) == ep.keys).all() and (h(dep.args, np.uint64) == ep.args).all()
            and (h(dep.types, np.uint8) == ep.types).all() and (h(dep.tables, np.uint8) == ep.tables).all()
            and (h(dep.acc_txn, np.uint32) == ep.acc_txn()).all()
            and (h(dep.txn_type, np.uint8) == ep.txn_type).all() and (h(dep.owner, np.uint8) == ep.owner).all()
            and (h(dep.client_startts, np.uint64) == ep.client_startts).all()
            and (h(dep.return_node, np.uint32) == ep.return_node).all()
            and int(dep.txn_id[-1].item()) == ing.next_txn - 1)

# per-kernel time of the resident ingest
eng.set_timing(False, profile=True)
eng.kernel_times(reset=True)
for _ in range(args.reps):
    leg_c()
kt = eng.kernel_times(reset=True)
eng.set_timing(False)

out_bytes = int(ep.n_acc) * (8 + 1 + 4 + 1 + 8 + 1) + n_txn * (4 + 1 + 8 + 8 + 4) + 8
out = {
    "txns": n_txn, "accesses": int(ep.n_acc), "batches": int(len(off) - 1), "wire_bytes": int(len(buf)),
    "epoch_bytes_written": out_bytes, "warehouses": args.wh, "stream_repeats": args.repeat,
    "device": torch.cuda.get_device_name(0), "reps": args.reps,
    "a_host_decode_plus_upload_ms": best["a"] * 1e3, "a_host_decode_alone_ms": best["a_decode"] * 1e3,
    "b_upload_bytes_plus_device_ingest_ms": best["b"] * 1e3,
    "c_device_ingest_resident_ms": best["c"] * 1e3,
    "runs_ms": {k: [round(x * 1e3, 3) for x in v] for k, v in runs.items()},
    "b_over_a": best["b"] / best["a"], "c_over_a": best["c"] / best["a"],
    "c_txns_per_s": n_txn / best["c"], "c_wire_GBps": len(buf) / best["c"] / 1e9,
    "a_decode_txns_per_s": n_txn / best["a_decode"],
    "kernels_us": {k: round(ms / n * 1e3, 2) for k, (n, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])},
    "device_epoch_equals_host_decoder": same, "src_hash": L.source_hash(),
    "note": "host clock around each leg, ending in a device synchronise; best of reps, legs alternated; "
            "uploads from pageable host memory, as T.device_epoch(ep) does",
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
