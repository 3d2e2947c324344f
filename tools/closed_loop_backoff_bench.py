"""What exponential back-off (dv_closed_loop_backoff, dvcc.LoopBackoff) does to
the device closed loop at config D (16,777,216 rows, 1,048,576-txn epochs,
NO_WAIT, zipf 0.9) on one context: the tracked plain loop and back-off at
D = 2, 4, 8 alternated in one process -- `--rounds` rounds of `--warmup` +
`--epochs` epochs per leg, every run a fresh loop from cursor 0 over the same
pool with an empty ring.  The run is longer than closed_loop_track_bench's: a
longest delay of D epochs needs several multiples of D epochs to reach its
steady state.  Per leg: ms per epoch and committed txns per second over the
timed epochs, with the commit and abort totals they come from, aborts per
commit, the mean (k - born) at commit, entries spilled per epoch, and the
fullest the ring got.  The headline is committed txns/s against the plain
loop's, same process, same box.  A last run per leg collects the per-launch
kernel averages (DV_FLAG_KERNEL_PROFILE) of the refill's launches.  Prints
one JSON line; `--out FILE` keeps it.

`--lanes L` (L > 1) measures the same legs on the closed loop over L decision
lanes (dv_epoch_run_closed_loop_lanes under dv_closed_loop_backoff_lanes: one
ring shared by the lanes, a txn's a-th abort costing L - 1 + min(2^(a-1), D)
epochs) against the tracked plain lanes loop, whose every retry comes L
epochs later; `--warmup` and `--epochs` are rounded up to multiples of 2 L
(a resumed call continues each lane in its first buffer).

`--tpcc` measures the same legs on the TPC-C closed loop
(dv_tpcc_epoch_run_closed_loop under dv_tpcc_closed_loop_backoff,
dvcc.TpccLoopBackoff) with bench.py's config-E parameters: `--tpcc-wh`
warehouses (32), `--cc` (WAIT_DIE), 65,536 txns per epoch unless `--n-txn`
says otherwise, a pool of two epochs' txns.  With `--lanes L` it is the TPC-C
loop over L decision lanes (dv_tpcc_epoch_run_closed_loop_lanes under
dv_tpcc_closed_loop_backoff_lanes), the legs and the rounding as for the YCSB
lanes loop."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "deneva-plus_amd"))
import dvcc  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=16_777_216)
    ap.add_argument("--n-txn", type=int, default=None, help="txns per epoch (1,048,576; --tpcc: 65,536)")
    ap.add_argument("--slots", type=int, nargs="*", default=[2, 4, 8])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=40)
    ap.add_argument("--lanes", type=int, default=1)
    ap.add_argument("--tpcc", action="store_true", help="the TPC-C closed loop at config E")
    ap.add_argument("--tpcc-wh", type=int, default=32)
    ap.add_argument("--cc", default="WAIT_DIE", help="--tpcc: NO_WAIT, WAIT_DIE or OCC")
    ap.add_argument("--out")
    a = ap.parse_args()
    nl = max(1, a.lanes)
    n_txn = a.n_txn if a.n_txn else (65_536 if a.tpcc else 1_048_576)
    if nl > 1:
        a.warmup, a.epochs = (-(-v // (2 * nl)) * 2 * nl for v in (a.warmup, a.epochs))
    if a.tpcc:  # (both set-ups: the pool uploaded before the engine's stream is made current)
        from dvcc import tpcc as T
        tp = T.tpcc_params(a.tpcc_wh)
        pool = T.gen(tp, 2 * n_txn, dvcc.epoch_seed(0, 999))
        dpool, pargs = T.device_epoch(pool)
        pb = torch.from_numpy(pool.txn_begin.astype("int32")).cuda()
        torch.cuda.set_stream(torch.cuda.Stream())
        eng = T.TpccEngine(a.cc, tp, n_txn, seed=1)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        ring = lambda trk, D: T.TpccLoopBackoff(trk, D, lanes=nl)  # noqa: E731
        what = {"warehouses": a.tpcc_wh, "cc": a.cc, "pool_txns": pool.n_txn, "max_txn_acc": int(dpool.max_txn_acc)}
    else:
        gen = dvcc.YCSBQueryGenerator(a.rows, part_cnt=1, req_per_query=10, zipf_theta=0.9, txn_write_perc=1.0,
                                      tup_write_perc=0.5, part_per_txn=1, strict_ppt=1, mpr=-1.0)
        pool = gen.gen(2 * n_txn, dvcc.epoch_seed(0, 999))
        dpool = dvcc.DeviceEpoch(pool)
        pb = torch.from_numpy(pool.txn_begin.astype("int32")).cuda()
        torch.cuda.set_stream(torch.cuda.Stream())
        eng = dvcc.CCEngine("NO_WAIT", n_txn, n_txn * 10)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.load_ycsb_partition(a.rows)
        ring, what = dvcc.LoopBackoff, {"rows": a.rows}
    lanes = [eng.open_lane() for _ in range(nl - 1)]
    total = a.warmup + a.epochs
    trk = dvcc.LoopTrack(n_txn, 2 * nl, log_cap=n_txn * total, epoch_cap=total, n_bins=64)
    rings = {D: ring(trk, D) for D in a.slots}
    # (the lanes decide epochs side by side: a commit array per epoch in flight)
    d_commit = torch.zeros(n_txn, dtype=torch.uint8, device="cuda") if nl == 1 else \
        [torch.zeros(n_txn, dtype=torch.uint8, device="cuda") for _ in range(2 * nl)]
    bufs = None

    def loop(n, cursor, resume):
        if a.tpcc and nl > 1:
            return eng.closed_loop_lanes(lanes, dpool, pargs, pb, n_txn, n, cursor=cursor, bufs=bufs,
                                         d_commits=[d_commit[k % (2 * nl)] for k in range(n)], resume=resume,
                                         track=trk)
        if a.tpcc:
            return eng.closed_loop(dpool, pargs, pb, n_txn, n, cursor=cursor, bufs=bufs, d_commits=d_commit,
                                   resume=resume, track=trk)
        if nl == 1:
            return eng.closed_loop(dpool, pb, n_txn, n, cursor=cursor, bufs=bufs, d_commits=d_commit, resume=resume,
                                   track=trk)
        return eng.closed_loop_lanes(lanes, dpool, pb, n_txn, n, cursor=cursor, bufs=bufs,
                                     d_commits=[d_commit[k % (2 * nl)] for k in range(n)], resume=resume, track=trk)

    def run(D):
        """a fresh loop under back-off D (None: the tracked plain loop)"""
        nonlocal bufs
        for t in [trk.log_pos, trk.epoch_end, trk.hist, trk.tot] + trk.ids:
            t.zero_()
        trk.attach(eng)
        bo = rings.get(D)
        if bo is not None:
            for t in [bo.slot_count, bo.ctr] + bo.aborts:
                t.zero_()
            bo.attach(eng)

        def swap():  # (one context only: the lanes' calls are multiples of 2 L epochs)
            bufs.swap()
            trk.swap()
            if bo is not None:
                bo.swap()

        cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
        _, bufs, cursor = loop(a.warmup, cursor, False)
        if a.warmup & 1:
            swap()
        torch.cuda.synchronize()
        before = trk.totals() + (bo.counters() if bo is not None else [0, 0, 0, 0])
        t0 = time.perf_counter()
        sts, bufs, cursor = loop(a.epochs, cursor, True)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        if a.epochs & 1:
            swap()
        after = trk.totals() + (bo.counters() if bo is not None else [0, 0, 0, 0])
        committed, aborted = after[0] - before[0], after[1] - before[1]
        assert committed == sum(s.committed for s in sts) and aborted == sum(s.aborted for s in sts)
        hist = trk.histogram()
        if bo is not None:
            wait = after[6] - before[6]
            assert after[5] == 0, "entries lost: the ring's capacity bound does not hold"
            fullest = int(bo.slot_count.max().item())
        else:  # (every retry L epochs later: k - born is L times the retry count; all epochs, warm-up included)
            wait = None
            fullest = 0
        res = {"ms_per_epoch": round(sec / a.epochs * 1e3, 4), "committed_per_s": round(committed / sec, 1),
               "committed": committed, "aborted": aborted,
               "aborts_per_commit": round(aborted / committed, 3) if committed else None,
               "mean_wait_epochs": round(wait / committed, 3) if wait is not None and committed else None,
               "mean_aborts_at_commit_all_epochs": round(float((hist * range(len(hist))).sum()) / max(1, hist.sum()), 3),
               "max_aborts_at_commit": after[3], "spilled_per_epoch": round((after[4] - before[4]) / a.epochs, 1),
               "parked_at_end": after[7], "fullest_slot_at_end": fullest}
        trk.detach()  # (and the back-off with it)
        return res

    legs = [None] + list(a.slots)
    name = lambda D: "plain" if D is None else f"D{D}"  # noqa: E731
    out = {**what, "n_txn": n_txn, "decision_lanes": nl, "warmup": a.warmup, "epochs": a.epochs, "rounds": a.rounds,
           "source": dvcc._lib.source_hash(), "legs": {name(D): [] for D in legs}}
    for _ in range(a.rounds):
        for D in legs:
            out["legs"][name(D)].append(run(D))
    best = {k: max(r["committed_per_s"] for r in v) for k, v in out["legs"].items()}
    out["committed_per_s_vs_plain"] = {k: round(v / best["plain"], 3) for k, v in best.items()}
    out["ms_per_epoch_min"] = {k: min(r["ms_per_epoch"] for r in v) for k, v in out["legs"].items()}
    out["kernels_us"] = {}
    for D in legs:  # each leg's refill launches, each timed on its own
        eng.set_timing(False, profile=True)
        eng.kernel_times(reset=True)
        run(D)
        kt = eng.kernel_times(reset=True)
        eng.set_timing(False)
        out["kernels_us"][name(D)] = {k: round(ms / n * 1e3, 2)
                                      for k, (n, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])
                                      if k.startswith(("k_bo_", "k_track", "k_carry", "k_refill"))}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
