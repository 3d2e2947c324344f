"""Retrying aborted TPC-C txns at config E's one-GPU share (32 warehouses, full
item / customer counts, 65,536-txn epochs, WAIT_DIE): ms per epoch of

  device  dv_tpcc_epoch_run_closed_loop -- the next epoch (aborted txns, then
          fresh pool txns) is built on the device;
  host    the retry loop a caller had to write before it: one
          dv_tpcc_epoch_run_device per epoch, D2H of the commit bytes, the next
          epoch's five arrays rebuilt in numpy, H2D.

Both start from the same pool and cursor on engines loaded alike, so they run
the same epochs: every epoch's commit bytes are compared at the end.  After
the warm-up the timed epochs run in chunks, the two loops alternating, each
chunk under a host clock that ends in a device synchronise.  Prints one JSON
line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deneva-plus_amd"))
import dvcc  # noqa: E402
from dvcc import tpcc as T  # noqa: E402

MAX_TXN_ACC = 33  # NewOrder with 15 lines


def select(ep, ids):
    """txns `ids` of `ep`, in that order, as a TpccEpoch (five arrays)"""
    tb = ep.txn_begin.astype(np.int64)
    ids = np.asarray(ids, np.int64)
    lens = tb[ids + 1] - tb[ids]
    ntb = np.zeros(len(ids) + 1, np.int64)
    ntb[1:] = np.cumsum(lens)
    idx = np.repeat(tb[ids] - ntb[:-1], lens) + np.arange(int(ntb[-1]), dtype=np.int64)
    return T.TpccEpoch(ep.keys[idx], ep.types[idx], ntb.astype(np.uint32), ep.tables[idx], ep.args[idx])


def next_epoch(host, commit, pool, cur, n_txn):
    """the closed loop's rule on the host: `host`'s aborted txns in order, then
    fresh pool txns from `cur` on (wrapping); returns the epoch and the cursor"""
    hc = select(host, np.flatnonzero(commit[:host.n_txn] == 0)[:n_txn])
    fresh = n_txn - hc.n_txn
    ft = select(pool, (cur + np.arange(fresh)) % pool.n_txn)
    tb = np.concatenate([hc.txn_begin, ft.txn_begin[1:] + hc.txn_begin[-1]]).astype(np.uint32)
    nxt = T.TpccEpoch(np.concatenate([hc.keys, ft.keys]), np.concatenate([hc.types, ft.types]), tb,
                      np.concatenate([hc.tables, ft.tables]), np.concatenate([hc.args, ft.args]))
    return nxt, (cur + fresh) % pool.n_txn


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--num-wh", type=int, default=32)
    ap.add_argument("--cust-per-dist", type=int, default=3000)
    ap.add_argument("--max-items", type=int, default=100000)
    ap.add_argument("--n-txn", type=int, default=65536)
    ap.add_argument("--pool-epochs", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--chunk-epochs", type=int, default=5, help="timed epochs = chunks x chunk-epochs (20)")
    ap.add_argument("--cc", default="WAIT_DIE")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU path to time"
    n = a.n_txn
    pp = T.tpcc_params(num_wh=a.num_wh, cust_per_dist=a.cust_per_dist, max_items=a.max_items)
    pool = T.gen(pp, a.pool_epochs * n, dvcc.epoch_seed(0, 999))
    dpool, pargs = T.device_epoch(pool)
    dpool.max_txn_acc = MAX_TXN_ACC
    pb = torch.from_numpy(pool.txn_begin.astype(np.int32)).cuda()
    engs = {w: T.TpccEngine(a.cc, pp, n, seed=1) for w in ("device", "host")}
    total = a.warmup + a.chunks * a.chunk_epochs

    # the device loop's state, and one call of k epochs
    dv = dict(cursor=torch.zeros(1, dtype=torch.int32, device="cuda"), bufs=None, first=True, commits=[], sts=[])

    def device_epochs(k):
        cs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(k)]
        sts, dv["bufs"], dv["cursor"] = engs["device"].closed_loop(
            dpool, pargs, pb, n, k, cursor=dv["cursor"], bufs=dv["bufs"], d_commits=cs, resume=not dv["first"])
        if k & 1:
            dv["bufs"].swap()
        dv["first"] = False
        dv["commits"] += cs
        dv["sts"] += sts

    # the host-driven loop's
    first, cur = next_epoch(select(pool, []), np.zeros(0, np.uint8), pool, 0, n)
    hs = dict(host=first, cur=cur, dev=T.device_epoch(first), commits=[], sts=[])
    d_commit = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def host_epochs(k):
        for _ in range(k):
            dep, d_args = hs["dev"]
            hs["sts"].append(engs["host"].run_tpcc_epoch_device(dep, d_args, d_commit))
            commit = d_commit.cpu().numpy()  # D2H
            hs["commits"].append(commit.copy())
            hs["host"], hs["cur"] = next_epoch(hs["host"], commit, pool, hs["cur"], n)  # the numpy rebuild
            hs["dev"] = T.device_epoch(hs["host"])  # H2D

    def timed(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    device_epochs(a.warmup)
    host_epochs(a.warmup)
    ms = {"device": [], "host": []}
    for c in range(a.chunks):
        order = ("device", "host") if c % 2 == 0 else ("host", "device")
        for w in order:
            ms[w].append(timed(device_epochs if w == "device" else host_epochs, a.chunk_epochs))
    same = all(np.array_equal(dc.cpu().numpy(), hc) for dc, hc in zip(dv["commits"], hs["commits"]))
    assert len(dv["commits"]) == len(hs["commits"]) == total
    out = {"tool": "tpcc_closed_loop", "box": torch.cuda.get_device_name(0), "source_hash": dvcc._lib.source_hash(),
           "cc": a.cc, "num_wh": a.num_wh, "n_txn": n, "pool_txn": pool.n_txn, "warmup": a.warmup,
           "timed_epochs": a.chunks * a.chunk_epochs, "same_commits": bool(same),
           "cursor_device": int(dv["cursor"].item()), "cursor_host": int(hs["cur"])}
    for w, sts in (("device", dv["sts"]), ("host", hs["sts"])):
        t = sts[a.warmup:]
        committed = sum(s.committed for s in t)
        mean = float(np.mean(ms[w]))
        out[w] = {"ms_per_epoch": round(mean, 4), "chunks_ms": [round(x, 4) for x in ms[w]],
                  "committed_per_s": round(committed / (mean * 1e-3 * len(t)), 1),
                  "abort_rate": round(1.0 - committed / (n * len(t)), 5),
                  "acc_per_epoch": round(float(np.mean([s.n_acc for s in t])), 1)}
    out["device_over_host"] = round(out["device"]["ms_per_epoch"] / out["host"]["ms_per_epoch"], 4)
    print(json.dumps(out))
    for e in engs.values():
        e.close()
    if not same or out["cursor_device"] != out["cursor_host"]:
        sys.exit("the two loops did not run the same epochs")


if __name__ == "__main__":
    main()
