"""Config D's epoch from Deneva's wire format to a device-resident epoch, three
ways on one box: the epoch as runcl's client batches (CL_QRY
mbufs of at most 4 KB, tests/wire_fmt.ycsb_epoch_buffer_np), then, alternated
and best of three,
  (a) host decode (dv_wire_decode_batches, one core) + DeviceEpoch(ep) upload
      -- the path before the device ingress;
  (b) upload of the raw bytes + dv_wire_ingest_device;
  (c) dv_wire_ingest_device with the bytes already resident;
each timed by the host clock around work that ends in a device synchronise.
Then the ingest's per-kernel time (dv_kernel_times) and a check that the
device epoch equals the host decoder's.  Prints one JSON line.

    python tools/wire_ingest_bench.py [--txns N] [--reps R] [--out FILE]
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
from dvcc.wire import DeviceWireIngress, WireIngress  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--txns", type=int, default=1_048_576)
ap.add_argument("--rows", type=int, default=16_777_216)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

rows, n_txn = args.rows, args.txns
gen = dvcc.YCSBQueryGenerator(rows, part_cnt=1, req_per_query=10, zipf_theta=0.9, txn_write_perc=1.0,
                              tup_write_perc=0.5, part_per_txn=1, strict_ppt=1, mpr=-1.0)
epoch = gen.gen(n_txn, dvcc.epoch_seed(0, 7))
buf, off = W.ycsb_epoch_buffer_np(epoch, 0, 1)
buf = np.ascontiguousarray(buf)
off64 = torch.from_numpy(off.view(np.int64))

eng = dvcc.CCEngine("NO_WAIT", n_txn, epoch.n_acc)
eng.load_ycsb_partition(rows)
host = WireIngress(L.YCSB, n_txn, epoch.n_acc, node_id=0, node_cnt=1, synth_table_size=rows)
ing = DeviceWireIngress(eng, n_txn, epoch.n_acc, node_id=0, node_cnt=1, synth_table_size=rows)


def sync():
    torch.cuda.synchronize()


def leg_a():
    t0 = time.perf_counter()
    closed = host.feed_buffer(buf, off)
    ep = host.take()
    t1 = time.perf_counter()
    dep = dvcc.DeviceEpoch(ep)
    sync()
    t2 = time.perf_counter()
    assert not closed and ep.n_txn == n_txn
    return t2 - t0, t1 - t0, ep, dep


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
best = {"a": None, "a_decode": None, "b": None, "c": None}
keep = lambda k, v: best.__setitem__(k, v if best[k] is None else min(best[k], v))  # noqa: E731
for _ in range(args.reps):
    ta, tdec, ep, _dep = leg_a()
    keep("a", ta)
    keep("a_decode", tdec)
    keep("b", leg_b()[0])
    tc, dep = leg_c()
    keep("c", tc)

# the device epoch against the host decoder's
sync()
ing_next = ing.next_txn
same = bool(dep.n_txn == ep.n_txn and dep.n_acc == ep.n_acc
            and (dep.txn_begin[:ep.n_txn + 1].cpu().numpy().view(np.uint32) == ep.txn_begin).all()
            and (dep.recs32[:ep.n_acc].cpu().numpy().view(np.uint32) == ep.to_row_records()).all()
            and (dep.client_startts.cpu().numpy().view(np.uint64) == ep.client_startts).all()
            and (dep.return_node.cpu().numpy().view(np.uint32) == ep.return_node).all()
            and int(dep.txn_id[-1].item()) == ing_next - 1)
form = "records + boundaries" if eng.reads_tb_only(n_txn) else "records + boundaries + keys / types / txn ids"

# per-kernel time of the resident ingest
eng.set_timing(False, profile=True)
eng.kernel_times(reset=True)
for _ in range(args.reps):
    leg_c()
kt = eng.kernel_times(reset=True)
eng.set_timing(False)

# the decoded epoch decides as the generated one
d_commit = torch.zeros(n_txn, dtype=torch.uint8, device="cuda")
d_ref = torch.zeros(n_txn, dtype=torch.uint8, device="cuda")
dep, _, _ = ing.feed_buffer(d_buf, d_off)
st = eng.run_epoch_device(dep, d_commit)
eng.run_epoch_device(dvcc.DeviceEpoch(epoch), d_ref)
t0 = time.perf_counter()
replies = ing.respond(dep, d_commit)
t_rsp = time.perf_counter() - t0

out = {
    "txns": n_txn, "accesses": int(epoch.n_acc), "batches": int(len(off) - 1), "wire_bytes": int(len(buf)),
    "device": torch.cuda.get_device_name(0), "reps": args.reps, "form": form,
    "a_host_decode_plus_upload_ms": best["a"] * 1e3, "a_host_decode_alone_ms": best["a_decode"] * 1e3,
    "b_upload_bytes_plus_device_ingest_ms": best["b"] * 1e3,
    "c_device_ingest_resident_ms": best["c"] * 1e3,
    "b_over_a": best["b"] / best["a"], "c_over_a": best["c"] / best["a"],
    "c_txns_per_s": n_txn / best["c"], "c_wire_GBps": len(buf) / best["c"] / 1e9,
    "kernels_us": {k: round(ms / n * 1e3, 2) for k, (n, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])},
    "device_epoch_equals_host_decoder": same,
    "commit_bytes_equal_generated_epoch": bool((d_commit == d_ref).all().item()),
    "committed": int(st.committed), "prefix_txn": int(st.prefix_txn),
    "reply_batches": len(replies), "respond_ms": t_rsp * 1e3, "src_hash": L.source_hash(),
    "note": "host clock around each leg, ending in a device synchronise; best of reps, legs alternated; "
            "uploads from pageable host memory, as DeviceEpoch(ep) does",
}
line = json.dumps(out)
print(line)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
if not (same and out["commit_bytes_equal_generated_epoch"]):
    sys.exit(1)
