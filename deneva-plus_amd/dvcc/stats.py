"""Deneva-compatible statistics lines.

`summary_line` prints the counters this path owns in the format of
Stats_thd::print (statistics/stats.cpp:425-500) behind the "[summary] " /
"[prog] " prefix of Stats::print (stats.cpp:1541-1560), so Deneva's
scripts/helper.py (get_summary / process_results, helper.py:755-815, 934-944)
parses engine runs like rundb output.  Times are seconds, as the reference
prints them (x / BILLION).  Counters of subsystems outside this path
(network, queues, latency breakdowns) are not printed.

`summary_fields` sees only per-epoch counts, where an abort is an abort.  A
closed loop run with a tracker (dvcc.LoopTrack) knows each txn through its
retries: `retry_summary_fields` prints the same keys with Deneva's distinction
between total and unique aborts and with latencies that include the retries.
"""


def summary_fields(total_runtime_s, stats, multi_part_txn_cnt=0, parts_touched=None, epoch_seconds=None,
                   part_counts=True):
    """stats: dv_stats of the epochs run in total_runtime_s (one partition's
    view; committed/aborted are global per epoch, as every rank decides every
    txn).  multi_part_txn_cnt / parts_touched: over the COMMITTED txns, as
    TxnManager::commit_stats counts them (txn.cpp:581-587, 600-602); by default
    every committed txn touched one partition.  txn_run_time sums the
    committed txns' latencies (txn.cpp:580): an epoch's txns start together
    and commit when it is decided, so each one's latency is its epoch's time --
    epoch_seconds[e] when given, else the epoch's share of the run (a lower
    bound when epochs overlap on decision lanes).  part_counts=False leaves
    the four partition counters out (a partitioned run that did not count
    them: the one-partition default would understate them)."""
    txn_cnt = sum(int(s.committed) for s in stats)       # INC_STATS(txn_cnt) on commit (txn.cpp:578)
    aborts = sum(int(s.aborted) for s in stats)           # total_txn_abort_cnt (stats.cpp:447)
    started = sum(int(s.n_txn) for s in stats)
    writes = sum(int(s.write_cnt) for s in stats)
    run = float(total_runtime_s)
    if epoch_seconds is None:
        epoch_seconds = [run / len(stats)] * len(stats) if stats else []
    run_time = sum(int(s.committed) * float(e) for s, e in zip(stats, epoch_seconds))
    tput = txn_cnt / run if run > 0 else 0.0             # stats.cpp:436-437
    parts = txn_cnt if parts_touched is None else int(parts_touched)
    single = txn_cnt - int(multi_part_txn_cnt)
    out = [
        ("total_runtime", run),
        ("tput", tput),
        ("txn_cnt", txn_cnt),
        ("remote_txn_cnt", 0),
        ("local_txn_cnt", txn_cnt),
        ("local_txn_start_cnt", started),
        ("total_txn_commit_cnt", txn_cnt),
        ("local_txn_commit_cnt", txn_cnt),
        ("remote_txn_commit_cnt", 0),
        ("total_txn_abort_cnt", aborts),
        ("unique_txn_abort_cnt", aborts),
        ("local_txn_abort_cnt", aborts),
        ("remote_txn_abort_cnt", 0),
        ("txn_run_time", run_time),
        ("txn_run_avg_time", run_time / txn_cnt if txn_cnt else 0.0),
        ("multi_part_txn_cnt", int(multi_part_txn_cnt)),
        ("single_part_txn_cnt", single),
        ("txn_write_cnt", writes),
        ("record_write_cnt", writes),
        ("parts_touched", parts),
        ("avg_parts_touched", parts / txn_cnt if txn_cnt else 0.0),
    ]
    if not part_counts:
        drop = {"multi_part_txn_cnt", "single_part_txn_cnt", "parts_touched", "avg_parts_touched"}
        out = [kv for kv in out if kv[0] not in drop]
    return out


def summary_line(total_runtime_s, stats, prog=False, **kw):
    body = ",".join(f"{k}={v:f}" if isinstance(v, float) else f"{k}={v:d}"
                    for k, v in summary_fields(total_runtime_s, stats, **kw))
    return ("[prog] " if prog else "[summary] ") + body


def retry_summary_fields(total_runtime_s, stats, totals, hist, penalty_epochs, epoch_seconds=None,
                         wait_epochs=None, **kw):
    """summary_fields for a closed loop run under a loop tracker: the same keys,
    with what the tracker knows about retries.  totals / hist: LoopTrack.totals()
    (committed, aborted, first aborts, max retries) and LoopTrack.histogram()
    over the epochs of `stats`; penalty_epochs: epochs until an aborted txn runs
    again (1, or the lanes loop's lane count).
    unique_txn_abort_cnt is the first aborts: a txn aborted five times counts
    five in total_txn_abort_cnt and one here, as Stats_thd counts them
    (txn.cpp: unique_txn_abort_cnt only when the txn had not aborted before).
    txn_run_time charges a commit after r retries r * penalty_epochs + 1
    epochs of the mean epoch time (epoch_seconds' mean when given, else the
    run's share), from the histogram -- exact while no commit lands in its last,
    saturating bin (every commit there is charged n_bins - 1 retries: a lower
    bound); txn_run_avg_time divides by the commits.
    wait_epochs (a loop under back-off, LoopBackoff.counters()[2]: the sum over
    the commits of k - born): txn_run_time charges wait_epochs + commits epochs
    instead -- exact, whatever delays the retries took and with no saturating
    bin; penalty_epochs is then not used."""
    base = dict(summary_fields(total_runtime_s, stats, epoch_seconds=epoch_seconds, **kw))
    hist = [int(h) for h in hist]
    n_ep = len(stats)
    if epoch_seconds is not None and len(epoch_seconds):
        per = sum(float(e) for e in epoch_seconds) / len(epoch_seconds)
    else:
        per = float(total_runtime_s) / n_ep if n_ep else 0.0
    commits = sum(hist)
    if wait_epochs is not None:
        run_time = (int(wait_epochs) + commits) * per
    else:
        run_time = sum(h * (r * int(penalty_epochs) + 1) for r, h in enumerate(hist)) * per
    base["unique_txn_abort_cnt"] = int(totals[2])
    base["txn_run_time"] = run_time
    base["txn_run_avg_time"] = run_time / commits if commits else 0.0
    return list(base.items())


def retry_summary_line(total_runtime_s, stats, totals, hist, penalty_epochs, prog=False, **kw):
    body = ",".join(f"{k}={v:f}" if isinstance(v, float) else f"{k}={v:d}"
                    for k, v in retry_summary_fields(total_runtime_s, stats, totals, hist, penalty_epochs, **kw))
    return ("[prog] " if prog else "[summary] ") + body
