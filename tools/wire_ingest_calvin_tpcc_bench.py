"""A config-E sequencer stream from Deneva's wire format to device-resident
TPC-C epochs under CALVIN, three ways on one box: --txns
queries of dv_tpcc_gen_queries at config E's one-GPU share (32 warehouses) as a
sequencer's forwarded CL_QRY messages (TPCCClientQueryMessage with batch_id,
tests/wire_fmt.tpcc_query) ended by RDONE, packed into mbufs of at most 4 KB as
MessageThread packs them -- with --repeat R the same queries R times back to
back as Calvin batches 4 .. 4 + R - 1, a batch starting wherever the one before
it ended, inside an mbuf -- then, alternated and best of three,
  (a) host decode (dv_wire_decode_batches under a calvin = 1, DV_TPCC cfg, one
      core) + T.device_epoch upload of every epoch -- the path before this entry;
  (b) upload of the raw bytes + dv_wire_ingest_device_calvin_tpcc, one call an epoch;
  (c) dv_wire_ingest_device_calvin_tpcc with the bytes already resident;
each timed by the host clock around work that ends in a device synchronise and
reported per epoch.  Then the ingest's per-kernel time (dv_kernel_times) and a
check, in the run itself, that every array of every device epoch equals the
host decoder's.  The ingest takes the stream and its per-call words from the
context and the access lists from the parameters, so the context here holds no
TPC-C tables.  Prints one JSON line.

    python tools/wire_ingest_calvin_tpcc_bench.py [--txns N] [--repeat R] [--reps K] [--out FILE]
"""
import argparse
import json
import os
import struct
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
from dvcc.wire import CalvinTpccDeviceWireIngress, WireIngress, tpcc_gen_queries  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--txns", type=int, default=65_536)
ap.add_argument("--repeat", type=int, default=1, help="the queries as this many Calvin batches back to back")
ap.add_argument("--wh", type=int, default=32)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

n_txn, R, E0 = args.txns, args.repeat, 4
pp = T.tpcc_params(args.wh)
qs = tpcc_gen_queries(pp, n_txn, 7)
one = []
for i in range(n_txn):
    x = qs[i]
    one.append(W.tpcc_query(dict(
        txn_type=x.txn_type, w_id=x.w_id, d_id=x.d_id, c_id=x.c_id, d_w_id=x.d_w_id, c_w_id=x.c_w_id,
        c_d_id=x.c_d_id, c_last=bytes(x.c_last), h_amount=x.h_amount, by_last_name=x.by_last_name, ol_cnt=x.ol_cnt,
        o_entry_d=x.o_entry_d, parts=[x.parts[k] for k in range(x.n_parts)],
        items=[(x.items[k].ol_i_id, x.items[k].ol_supply_w_id, x.items[k].ol_quantity) for k in range(x.ol_cnt)]),
        client_startts=i, txn_id=2 * i, batch_id=E0))
del qs
msgs = []
for k in range(R):  # the same messages under batch id E0 + k (the header's third field, at byte 12)
    bid = struct.pack("<Q", E0 + k)
    msgs += [m[:12] + bid + m[20:] for m in one] if k else one
    msgs.append(W.rdone(E0 + k))
del one
mbufs = W.batches(0, 1, msgs)
del msgs
buf = np.frombuffer(b"".join(mbufs), np.uint8)
off = np.zeros(len(mbufs) + 1, np.uint64)
off[1:] = np.cumsum([len(b) for b in mbufs])
del mbufs
off64 = torch.from_numpy(off.view(np.int64))
max_acc = n_txn * (3 + 2 * pp.max_items_per_txn)

eng = dvcc.CCEngine("CALVIN", 1024, 1024)  # (the stream and the ingest's per-call words)
host = WireIngress(L.TPCC, n_txn, max_acc, calvin=True, tpcc=pp)
ing = CalvinTpccDeviceWireIngress(eng, pp, n_txn, max_acc)
ARRAYS = (("keys", np.uint64), ("types", np.uint8), ("tables", np.uint8), ("args", np.uint64), ("owner", np.uint8),
          ("txn_begin", np.uint32), ("txn_type", np.uint8), ("txn_id", np.uint64), ("client_startts", np.uint64),
          ("return_node", np.uint32))


def sync():
    torch.cuda.synchronize()


def leg_a():
    t0 = time.perf_counter()
    eps = host.feed_buffer(buf, off)
    eps.append(host.take())
    host.ready.clear()
    t1 = time.perf_counter()
    deps = [T.device_epoch(ep) for ep in eps]
    sync()
    t2 = time.perf_counter()
    assert len(eps) == R and all(ep.n_txn == n_txn and ep.rdone == 1 for ep in eps)
    return t2 - t0, t1 - t0, eps, deps


def ingest_all(d_buf, d_off, keep=False):
    """one call an epoch from the cursor; keep: clones of every epoch's arrays"""
    cur, kept = None, []
    for k in range(R):
        p = ing.feed_buffer(d_buf, d_off, cur)
        assert p.stop == (L.WIRE_STOP_END if k == R - 1 else L.WIRE_STOP_BATCH), (k, p.stop, p.batch, p.msg)
        cur = (p.batch, p.msg)
        dep = ing.take()
        assert (dep.n_txn, dep.rdone, dep.batch_id) == (n_txn, 1, E0 + k)
        if keep:
            kept.append({a: getattr(dep, a).clone() for a in [a for a, _ in ARRAYS] + ["acc_txn"]})
    return dep, kept


def leg_b():
    t0 = time.perf_counter()
    d_buf, d_off = torch.from_numpy(buf).to("cuda"), off64.to("cuda")
    dep, _ = ingest_all(d_buf, d_off)
    sync()
    return time.perf_counter() - t0, dep


d_buf, d_off = torch.from_numpy(buf).to("cuda"), off64.to("cuda")


def leg_c():
    sync()
    t0 = time.perf_counter()
    dep, _ = ingest_all(d_buf, d_off)
    sync()
    return time.perf_counter() - t0, dep


leg_a(), leg_b(), leg_c()  # warm-up of every leg
runs = {"a": [], "a_decode": [], "b": [], "c": []}
for _ in range(args.reps):
    ta, tdec, eps, _deps = leg_a()
    runs["a"].append(ta)
    runs["a_decode"].append(tdec)
    runs["b"].append(leg_b()[0])
    runs["c"].append(leg_c()[0])
del _deps
best = {k: min(v) for k, v in runs.items()}
c_below_decode = all(c < d for c, d in zip(runs["c"], runs["a_decode"]))

# every device epoch against the host decoder's, every array
_, kept = ingest_all(d_buf, d_off, keep=True)
sync()
u = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
same = all(bool(all((u(d[a], dt) == getattr(ep, a)).all() for a, dt in ARRAYS)
                and (u(d["acc_txn"], np.uint32) == ep.acc_txn()).all()) for d, ep in zip(kept, eps))
n_acc = int(eps[0].n_acc)
del kept

# per-kernel time of the resident ingest
eng.set_timing(False, profile=True)
eng.kernel_times(reset=True)
for _ in range(args.reps):
    leg_c()
kt = eng.kernel_times(reset=True)
eng.set_timing(False)

out = {
    "txns_per_epoch": n_txn, "epochs": R, "accesses_per_epoch": n_acc, "mbufs": int(len(off) - 1),
    "wire_bytes": int(len(buf)), "warehouses": args.wh, "device": torch.cuda.get_device_name(0), "reps": args.reps,
    "a_host_decode_plus_upload_ms_per_epoch": best["a"] / R * 1e3,
    "a_host_decode_alone_ms_per_epoch": best["a_decode"] / R * 1e3,
    "b_upload_bytes_plus_device_ingest_ms_per_epoch": best["b"] / R * 1e3,
    "c_device_ingest_resident_ms_per_epoch": best["c"] / R * 1e3,
    "runs_ms_per_epoch": {k: [round(x / R * 1e3, 4) for x in v] for k, v in runs.items()},
    "b_over_a": best["b"] / best["a"], "c_over_a": best["c"] / best["a"],
    "a_decode_over_c": best["a_decode"] / best["c"], "c_below_a_decode_in_every_pair": c_below_decode,
    "c_txns_per_s": n_txn * R / best["c"], "c_wire_GBps": len(buf) / best["c"] / 1e9,
    "a_decode_txns_per_s": n_txn * R / best["a_decode"],
    "kernels_us_per_launch": {k: round(ms / n * 1e3, 2) for k, (n, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])},
    "device_epochs_equal_host_decoder": same, "src_hash": L.source_hash(),
    "note": "host clock around each leg, ending in a device synchronise; best of reps, legs alternated; uploads "
            "from pageable host memory, as T.device_epoch(ep) does; a call of the ingest sees the stream's mbufs "
            "from its cursor to the end of its window, so with --repeat every call but the last checks mbufs of "
            "later batches too",
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
