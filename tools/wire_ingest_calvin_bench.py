"""Config B's epoch from a CALVIN sequencer's wire stream to a device-resident
epoch, three ways on one box: the epoch as the sequencer's
forwarded CL_QRY messages ended by RDONE, packed into mbufs of at most 4 KB as
MessageThread packs them -- with --repeat R the same queries R times back to
back as R Calvin batches, a batch starting wherever the one before it ended,
inside an mbuf -- then, alternated and best of three,
  (a) host decode (dv_wire_decode_batches under a CALVIN cfg, one core) +
      DeviceEpoch(ep) upload of every epoch -- the path before the device ingress;
  (b) upload of the raw bytes + dv_wire_ingest_device_calvin, one call an epoch;
  (c) dv_wire_ingest_device_calvin with the bytes already resident;
each timed by the host clock around work that ends in a device synchronise and
reported per epoch.  Then the ingest's per-kernel time (dv_kernel_times), the
check kernel's wire bytes per second, and a check that every array of the
device epochs equals the host decoder's and that a CALVIN engine gives the
ingested epoch the host-decoded epoch's grant groups.  Prints one JSON line.

    python tools/wire_ingest_calvin_bench.py [--txns N] [--repeat R] [--reps K] [--out FILE]
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
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402
from dvcc.wire import CalvinDeviceWireIngress, WireIngress  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--txns", type=int, default=65_536)
ap.add_argument("--rows", type=int, default=16_777_216)
ap.add_argument("--repeat", type=int, default=1)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

rows, n_txn, R = args.rows, args.txns, args.repeat
CL_QRY, RDONE, MSG_MAX, U64 = 3, 19, 4096, (1 << 64) - 1
gen = dvcc.YCSBQueryGenerator(rows, part_cnt=1, req_per_query=10, zipf_theta=0.6, txn_write_perc=1.0,
                              tup_write_perc=0.5, part_per_txn=1, strict_ppt=1, mpr=-1.0)
epoch = gen.gen(n_txn, dvcc.epoch_seed(0, 7))


def sequencer_stream(ep, first_batch_id, repeat, dest=0, src=1):
    """(uint8 array, uint64 offsets): the epoch's queries as one sequencer's
    CL_QRY messages (Message header with batch_id, transport/message.cpp:248-270)
    and an RDONE, `repeat` times with rising batch ids, packed greedily into
    mbufs (msg_thread.cpp:90-103)"""
    q = int(ep.txn_begin[1] - ep.txn_begin[0])
    assert (np.diff(ep.txn_begin.astype(np.int64)) == q).all()
    req = np.dtype([("acc", "<u4"), ("pad", "<u4"), ("key", "<u8"), ("val", "u1"), ("pad2", "u1", (7,))])
    msg = np.dtype([("rtype", "<u4"), ("txn_id", "<u8"), ("batch_id", "<u8"), ("mq", "<u8"), ("lat", "<f8", (7,)),
                    ("cst", "<u8"), ("np", "<u8"), ("part", "<u8"), ("nreq", "<u8"), ("req", req, (q,))], align=False)
    n = ep.n_txn
    m = np.zeros(n, dtype=msg)
    m["rtype"], m["np"], m["part"], m["nreq"] = CL_QRY, 1, 0, q
    m["req"]["acc"] = ep.types.reshape(n, q)
    m["req"]["key"] = ep.keys.reshape(n, q)
    flat, sizes = [], []
    for k in range(repeat):
        m["batch_id"] = first_batch_id + k
        m["txn_id"] = (k * n + np.arange(n, dtype=np.uint64)) * 2
        m["cst"] = 1_000_000 * k + np.arange(n, dtype=np.uint64)
        flat.append(m.view(np.uint8).reshape(-1).copy())
        flat.append(np.frombuffer(struct.pack("<IQQ", RDONE, U64, first_batch_id + k) + b"\0" * 64, np.uint8))
        sizes.append(np.full(n, msg.itemsize, np.int64))
        sizes.append(np.array([84], np.int64))
    flat, sizes = np.concatenate(flat), np.concatenate(sizes)
    moff = np.concatenate([[0], np.cumsum(sizes)])
    pieces, lens, i = [], [], 0
    while i < len(sizes):
        # the most messages from i that fit MSG_MAX - 12 bytes
        j = int(np.searchsorted(moff, moff[i] + MSG_MAX - 12, side="right")) - 1
        pieces.append(np.frombuffer(struct.pack("<III", dest, src, j - i), np.uint8))
        pieces.append(flat[moff[i]:moff[j]])
        lens.append(12 + int(moff[j] - moff[i]))
        i = j
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return np.ascontiguousarray(np.concatenate(pieces)), off


E0 = 4
buf, off = sequencer_stream(epoch, E0, R)
off64 = torch.from_numpy(off.view(np.int64))
n_mbufs = len(off) - 1

eng = dvcc.CCEngine("CALVIN", n_txn, epoch.n_acc)
eng.load_ycsb_partition(rows)
kw = dict(node_id=0, node_cnt=1, synth_table_size=rows)
host = WireIngress(L.YCSB, n_txn, epoch.n_acc, calvin=True, **kw)
ing = CalvinDeviceWireIngress(eng, n_txn, epoch.n_acc, **kw)


def sync():
    torch.cuda.synchronize()


def leg_a():
    t0 = time.perf_counter()
    eps = host.feed_buffer(buf, off)
    eps.append(host.take())
    host.ready.clear()
    t1 = time.perf_counter()
    deps = [dvcc.DeviceEpoch(ep) for ep in eps]
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
            kept.append({a: getattr(dep, a).clone() for a in ("keys", "types", "acc_txn", "txn_begin", "txn_id",
                                                               "client_startts", "return_node")})
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
best = {"a": None, "a_decode": None, "b": None, "c": None}
runs = {"a": [], "b": [], "c": []}
keep = lambda k, v: best.__setitem__(k, v if best[k] is None else min(best[k], v))  # noqa: E731
for _ in range(args.reps):
    ta, tdec, eps, _deps = leg_a()
    keep("a", ta)
    keep("a_decode", tdec)
    tb = leg_b()[0]
    keep("b", tb)
    tc, dep = leg_c()
    keep("c", tc)
    for k, v in (("a", ta), ("b", tb), ("c", tc)):
        runs[k].append(round(v / R * 1e3, 4))

# every device epoch against the host decoder's
_, kept = ingest_all(d_buf, d_off, keep=True)
sync()
u = lambda t, dt: t.cpu().numpy().view(dt)  # noqa: E731
same = all(bool((u(d["keys"], np.uint64) == ep.keys).all() and (u(d["types"], np.uint8) == ep.types).all()
                and (u(d["acc_txn"], np.uint32) == ep.acc_txn()).all()
                and (u(d["txn_begin"], np.uint32) == ep.txn_begin).all()
                and (u(d["txn_id"], np.uint64) == ep.txn_id).all()
                and (u(d["client_startts"], np.uint64) == ep.client_startts).all()
                and (u(d["return_node"], np.uint32) == ep.return_node).all()) for d, ep in zip(kept, eps))
del kept

# per-kernel time of the resident ingest
eng.set_timing(False, profile=True)
eng.kernel_times(reset=True)
for _ in range(args.reps):
    leg_c()
kt = eng.kernel_times(reset=True)
eng.set_timing(False)
kernels_us = {k: round(ms / n * 1e3, 2) for k, (n, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])}
check_us = kernels_us.get("k_wire_check_calvin")

# the ingested epoch's grant groups against the host-decoded epoch's (the last batch)
d_commit = torch.zeros(n_txn, dtype=torch.uint8, device="cuda")
d_grant = torch.zeros(epoch.n_acc, dtype=torch.int32, device="cuda")
r_commit, r_grant = torch.zeros_like(d_commit), torch.zeros_like(d_grant)
dep, _ = ingest_all(d_buf, d_off)
st = eng.run_epoch_device(dep, d_commit, d_grant)
eng.run_epoch_device(dvcc.DeviceEpoch(eps[-1]), r_commit, r_grant)
sync()
grants = bool((d_grant == r_grant).all().item() and (d_commit == r_commit).all().item())
t0 = time.perf_counter()
acks = ing.respond(dep)
t_rsp = time.perf_counter() - t0

wire_per_epoch = len(buf) / R
out = {
    "txns_per_epoch": n_txn, "epochs": R, "accesses_per_epoch": int(epoch.n_acc), "mbufs": int(n_mbufs),
    "wire_bytes": int(len(buf)), "device": torch.cuda.get_device_name(0), "reps": args.reps,
    "a_host_decode_plus_upload_ms_per_epoch": best["a"] / R * 1e3,
    "a_host_decode_alone_ms_per_epoch": best["a_decode"] / R * 1e3,
    "b_upload_bytes_plus_device_ingest_ms_per_epoch": best["b"] / R * 1e3,
    "c_device_ingest_resident_ms_per_epoch": best["c"] / R * 1e3,
    "b_over_a": best["b"] / best["a"], "c_over_a": best["c"] / best["a"],
    "c_txns_per_s": n_txn * R / best["c"], "c_wire_GBps": len(buf) / best["c"] / 1e9,
    "runs_ms_per_epoch": runs, "kernels_us_per_launch": kernels_us,
    "check_kernel_wire_GBps": None if not check_us else round(wire_per_epoch / (check_us * 1e-6) / 1e9, 2),
    "device_epochs_equal_host_decoder": same,
    "grant_groups_equal_host_decoded_epoch": grants,
    "committed": int(st.committed), "ack_batches": len(acks), "respond_ms": t_rsp * 1e3,
    "src_hash": L.source_hash(),
    "note": "host clock around each leg, ending in a device synchronise; best of reps, legs alternated; uploads "
            "from pageable host memory, as DeviceEpoch(ep) does; a call of the ingest sees the stream's mbufs "
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
if not (same and grants):
    sys.exit(1)
