"""k_bucket_sort's per-bucket time and per-launch span: config D with the
DVCC_BUCKET_STAMPS measurement build (tools/exp_variant.sh bstamps
dvcc_kernels.hip -DDVCC_BUCKET_STAMPS; run with
DVCC_LIB=exp_build/bstamps/libdvcc.so).  Thread 0 of every bucket's
workgroup stamps its start and end with the 100-MHz wall clock; per context
the build keeps every launch's span, from its first workgroup's start to its
last workgroup's end.

    exp_bucket_stamps.py [epochs] [lanes]

lanes = 1: one context; lanes = 4: the bench's four decision lanes, all
deciding (the spans are then per lane).  Prints one JSON line: the launch
span, the launch's slowest bucket against the mean bucket, and the buckets'
time against their key counts."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deneva-plus_amd"))
import dvcc  # noqa: E402
from dvcc import _lib as L  # noqa: E402

SLOTS = 8  # dvcc_kernels.hip kStampSlots
rows, n_txn = 16_777_216, 1_048_576
epochs = int(sys.argv[1]) if len(sys.argv) > 1 else 20
lanes_n = int(sys.argv[2]) if len(sys.argv) > 2 else 1
gen = dvcc.YCSBQueryGenerator(rows, part_cnt=1, req_per_query=10, zipf_theta=0.9, txn_write_perc=1.0,
                              tup_write_perc=0.5, part_per_txn=1, strict_ppt=1, mpr=-1.0)
eps = [gen.gen(n_txn, dvcc.epoch_seed(0, e)) for e in range(3)]
deps = [dvcc.DeviceEpoch(e) for e in eps]
eng = dvcc.CCEngine("NO_WAIT", n_txn, n_txn * 10)
eng.set_stream(torch.cuda.current_stream().cuda_stream)
eng.load_ycsb_partition(rows)
lanes = [eng.open_lane() for _ in range(lanes_n - 1)]
d = torch.zeros(n_txn, dtype=torch.uint8, device="cuda")
lib = L.lib()
lib.dv_debug_bucket_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
buf = np.zeros(1024 * 4, np.uint64)
lrec = np.zeros(4 + SLOTS * 8, np.uint64)


def run(k):
    batch = [deps[i % 3] for i in range(k)]
    return eng.run_epochs_lanes(lanes, batch, d) if lanes else eng.run_epochs_device(batch, d)


run(8)
assert lib.dv_debug_bucket_stamps(buf.ctypes.data, lrec.ctypes.data) == 0
run(epochs)
torch.cuda.synchronize()
assert lib.dv_debug_bucket_stamps(buf.ctypes.data, lrec.ctypes.data) == 0
w = buf.reshape(1024, 4).astype(np.float64)
used = w[:, 0] > 0
w = w[used]
us = w[:, 1] / w[:, 0] * 0.01
keys = w[:, 2] / w[:, 0]
order = np.argsort(keys)
dec = [{"keys": float(keys[order[i]]), "us": float(us[order[i]])}
       for i in np.linspace(0, len(order) - 1, 12).astype(int)]
nl = max(1, int(lrec[0]))
ctx = lrec[4:].reshape(SLOTS, 8)
ctx = ctx[ctx[:, 0] > 0]
spans = [{"launches": int(c[0]), "span_us_mean": float(c[1]) / float(c[0]) * 0.01, "span_us_max": float(c[2]) * 0.01}
         for c in ctx]
out = {"epochs": epochs, "lanes": lanes_n, "buckets": int(used.sum()), "launches": int(lrec[0]),
       "launch_span_us_mean": float(ctx[:, 1].sum()) / max(1.0, float(ctx[:, 0].sum())) * 0.01,
       "launch_span_by_context": spans,
       "launch_slowest_bucket_us": float(lrec[1]) / nl * 0.01, "launch_slowest_bucket_keys": float(lrec[2]) / nl,
       "bucket_us_mean": float(us.mean()), "bucket_keys_mean": float(keys.mean()),
       "bucket_us_max_mean": float(us.max()), "keys_of_slowest_mean_bucket": float(keys[np.argmax(us)]),
       "us_vs_keys_fit": [float(v) for v in np.polyfit(keys, us, 1)], "by_size": dec}
print(json.dumps(out))
for ln in lanes:
    ln.close()
eng.close()
