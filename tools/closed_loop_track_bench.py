"""What the loop tracker (dv_closed_loop_track, dvcc.LoopTrack) costs at config D
(16,777,216 rows, 1,048,576-txn epochs, NO_WAIT, zipf 0.9): the device closed
loop tracked and untracked, alternated in one process -- `--pairs` pairs of
`--warmup` + `--epochs` epochs each, every run a fresh loop from cursor 0 over
the same pool, so both forms decide the same epochs.  `--mode one` is one
context (dv_epoch_run_closed_loop), `--mode lanes` four decision lanes
(dv_epoch_run_closed_loop_lanes); run each mode as its own step under its own
`timeout`.  Checks that the tracked and the untracked loop leave equal commit
bytes (the last epoch's), committed counts and cursor, and that the tracker's
totals add up to the loop's statistics.  `--mode one` adds the tracked loop's
per-launch kernel averages (DV_FLAG_KERNEL_PROFILE), the two tracker kernels
among them.  Prints one JSON line; `--out FILE` keeps it."""
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
    ap.add_argument("--mode", choices=("one", "lanes"), default="one")
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--rows", type=int, default=16_777_216)
    ap.add_argument("--n-txn", type=int, default=1_048_576)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    n_txn, L = a.n_txn, (a.lanes if a.mode == "lanes" else 1)
    if a.mode == "lanes" and a.warmup % (2 * L):
        a.warmup += 2 * L - a.warmup % (2 * L)  # (resume: whole turns of the lanes' buffer pairs before it)
    gen = dvcc.YCSBQueryGenerator(a.rows, part_cnt=1, req_per_query=10, zipf_theta=0.9, txn_write_perc=1.0,
                                  tup_write_perc=0.5, part_per_txn=1, strict_ppt=1, mpr=-1.0)
    pool = gen.gen(2 * n_txn, dvcc.epoch_seed(0, 999))
    dpool = dvcc.DeviceEpoch(pool)
    pb = torch.from_numpy(pool.txn_begin.astype("int32")).cuda()
    torch.cuda.set_stream(torch.cuda.Stream())
    eng = dvcc.CCEngine("NO_WAIT", n_txn, n_txn * 10)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.load_ycsb_partition(a.rows)
    lanes = [eng.open_lane() for _ in range(L - 1)]
    total = a.warmup + a.epochs
    trk = dvcc.LoopTrack(n_txn, 2 * L, log_cap=n_txn * total, epoch_cap=total, n_bins=64)
    d_commit = torch.zeros(n_txn, dtype=torch.uint8, device="cuda")
    bufs = None

    def loop(n, cursor, resume, track):
        nonlocal bufs
        if L == 1:
            sts, bufs, cursor = eng.closed_loop(dpool, pb, n_txn, n, cursor=cursor, bufs=bufs, d_commits=d_commit,
                                                resume=resume, track=track)
        else:
            sts, bufs, cursor = eng.closed_loop_lanes(lanes, dpool, pb, n_txn, n, cursor=cursor, bufs=bufs,
                                                      d_commits=d_commit, resume=resume, track=track)
        return sts, cursor

    def run(tracked):
        """a fresh loop: warm-up, then the timed epochs -> (ms per epoch, stats, cursor, last commit bytes)"""
        if tracked:
            for t in (trk.log_pos, trk.epoch_end, trk.hist, trk.tot):
                t.zero_()
            trk.attach(eng)
        cursor = torch.zeros(1, dtype=torch.int32, device="cuda")
        w_sts, cursor = loop(a.warmup, cursor, False, trk if tracked else None)
        if L == 1 and a.warmup & 1:
            bufs.swap()
            if tracked:
                trk.swap()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sts, cursor = loop(a.epochs, cursor, True, trk if tracked else None)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / a.epochs * 1e3
        if L == 1 and a.epochs & 1:
            bufs.swap()
            if tracked:
                trk.swap()
        res = (ms, w_sts + sts, int(cursor.item()), d_commit.clone())
        if tracked:
            trk.detach()
        return res

    out = {"mode": a.mode, "lanes": L, "rows": a.rows, "n_txn": n_txn, "warmup": a.warmup, "epochs": a.epochs,
           "source": dvcc._lib.source_hash(), "untracked_ms": [], "tracked_ms": []}
    for _ in range(a.pairs):
        ms_u, sts_u, cur_u, c_u = run(False)
        ms_t, sts_t, cur_t, c_t = run(True)
        out["untracked_ms"].append(round(ms_u, 4))
        out["tracked_ms"].append(round(ms_t, 4))
        assert cur_u == cur_t, "the tracked loop's cursor differs"
        assert torch.equal(c_u, c_t), "the tracked loop's commit bytes differ"
        assert [s.committed for s in sts_u] == [s.committed for s in sts_t]
        committed, aborted, first, most = trk.totals()
        assert committed == sum(s.committed for s in sts_t) and aborted == sum(s.aborted for s in sts_t)
        assert int(trk.log_pos.item()) == committed and int(trk.hist.sum().item()) == committed
        out["tracker"] = {"committed": committed, "aborted": aborted, "first_aborts": first, "max_retries": most,
                          "hist": [int(h) for h in trk.histogram()[:most + 1]]}
    out["delta_us"] = round((min(out["tracked_ms"]) - min(out["untracked_ms"])) * 1e3, 2)
    if L == 1:  # the tracked loop's launches, each timed on its own
        eng.set_timing(False, profile=True)
        eng.kernel_times(reset=True)
        run(True)
        kt = eng.kernel_times(reset=True)
        eng.set_timing(False)
        out["kernels_us"] = {k: round(ms / n * 1e3, 2) for k, (n, ms) in sorted(kt.items(), key=lambda kv: -kv[1][1])
                             if k.startswith(("k_track", "k_carry", "k_refill"))}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    for ln in lanes:
        ln.close()
    eng.close()


if __name__ == "__main__":
    main()
