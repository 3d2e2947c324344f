"""bench.py's stdout record: one compact JSON line that
the driver parses -- the headline keys, the dominant kernel's roofline and the
CPU baseline -- with kernel tables and leg detail in the side file.  Built
from round 4's full 29.7-KB record (which the driver could not parse) and from
a synthetic N>1 record; no GPU.  Beside them the plain run (no --full): its
record, --dump-outputs on a stand-in engine, and one short run on the GPU."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL = os.path.join(ROOT, "profiles", "r04_final3", "bench.json")
REQUIRED = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline")


def _check(line, out):
    assert "\n" not in line and len(line) < bench.LINE_LIMIT, len(line)
    rec = json.loads(line)
    for k in REQUIRED:
        assert k in rec, k
    assert rec["value"] == pytest.approx(out["value"], rel=1e-3)
    assert rec["ms_per_step"] == pytest.approx(out["ms_per_step"], rel=1e-3)
    rf = rec["roofline"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "bytes_per_launch",
              "avg_launch_ms", "launches_per_epoch"):
        assert k in rf, k
    assert rf["kernel"] == out["roofline"]["kernel"]
    assert rf["frac"] == pytest.approx(out["roofline"]["frac"], rel=1e-3)
    for k in ("value", "unit", "cores", "kind"):
        assert k in rec["cpu_baseline"], k
    return rec


@pytest.mark.skipif(not os.path.exists(FULL), reason="round-4 record not in the tree")
def test_round4_record_compacts_under_the_limit(tmp_path):
    out = json.load(open(FULL))
    assert len(json.dumps(out)) > 20_000  # (the line the driver could not parse)
    path = bench.write_detail(out, str(tmp_path / "detail.json"))
    rec = _check(bench.headline_record(out, path), out)
    assert json.load(open(tmp_path / "detail.json")) == out
    legs = rec["legs"]
    assert legs["config_b"]["ms_per_epoch"] == pytest.approx(out["config_b"]["ms_per_epoch"], rel=1e-3)
    assert legs["config_c"]["roofline"]["kernel"] == out["config_c"]["roofline"]["kernel"]
    assert legs["tpcc"]["WAIT_DIE"]["ms_per_epoch"] == pytest.approx(out["tpcc"]["WAIT_DIE"]["ms_per_epoch"],
                                                                     rel=1e-3)
    assert "window_10000_CALVIN" in legs["tpcc"]
    assert legs["cpu_config_a"]["cores"] == 4


def test_plain_record_is_the_headline_alone():
    """A run without --full: the contract's keys and the config, no roofline,
    legs, CPU baseline or detail file."""
    out = {"metric": bench.METRIC, "value": 1.4e8, "unit": "committed txns/s", "n_gpus": 1, "steps": 20,
           "warmup": 5, "ms_per_step": 0.1768, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "u64", "data": "synthetic", "config": {"workload": "w", "cc_alg": "NO_WAIT"},
           "abort_rate": 0.977, "decided_txns_per_s": 5.9e9, "src_hash": "abc", "deneva_summary": "[summary] x"}
    line = bench.headline_record(out)
    assert "\n" not in line and len(line) < bench.LINE_LIMIT
    rec = json.loads(line)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"):
        assert rec[k] == pytest.approx(out[k], rel=1e-3) if isinstance(out[k], float) else rec[k] == out[k], k
    for k in ("roofline", "legs", "cpu_baseline", "detail"):
        assert k not in rec, k


def test_full_is_opt_in(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, "", 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


def test_dump_outputs_files(tmp_path):
    """--dump-outputs on a stand-in engine: float32 / float64 arrays, u64
    values exact as 32-bit halves, the same rows sampled every time."""
    import numpy as np
    import torch
    rows = 1 << 20

    class Eng:
        def read_table(self, first, n):
            return (np.arange(first, first + n, dtype=np.uint64) << np.uint64(40)) | np.uint64(0xFFFFFFFF)

    class St:
        n_txn, n_acc, committed, aborted, write_cnt, read_digest = 1000, 10_000, 3, 997, 15, (1 << 64) - 2

    commit = torch.zeros(1024, dtype=torch.uint8)
    commit[[1, 5, 999]] = 1
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), St, commit, 1000, Eng(), rows)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["commit.npy", "stats.npy", "table_f0.npy", "table_rows.npy"]
    assert all(v.dtype in (np.float32, np.float64) for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    assert got["commit.npy"].shape == (1000,) and got["commit.npy"].sum() == 3
    assert got["stats.npy"].tolist() == [1000, 10_000, 3, 997, 15, 0xFFFFFFFF, 0xFFFFFFFE]
    r = got["table_rows.npy"].astype(np.uint64)
    n = bench.DUMP_HOT_ROWS + bench.DUMP_BLOCKS * bench.DUMP_BLOCK_ROWS
    assert r.shape == (n,) and r.max() < rows and (r[:bench.DUMP_HOT_ROWS] == np.arange(bench.DUMP_HOT_ROWS)).all()
    f0 = got["table_f0.npy"].astype(np.uint64)
    assert f0.shape == (n, 2)
    assert (((f0[:, 0] << np.uint64(32)) | f0[:, 1]) == Eng().read_table(0, rows)[r]).all()
    for f, v in got.items():
        assert (np.load(tmp_path / "b" / f) == v).all(), f


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps(tmp_path):
    """bench.py as every pull request runs it: one JSON line on stdout, K timed
    steps, no side legs, and the last step's outputs consistent with each other."""
    import subprocess
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120,
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert (rec["metric"], rec["unit"], rec["dtype"], rec["higher_is_better"]) == \
        (bench.METRIC, "committed txns/s", "u64", True)
    assert (rec["steps"], rec["warmup"], rec["n_gpus"]) == (3, 1, 1)
    assert rec["ms_per_step"] > 0
    n_txn = rec["config"]["txns_per_epoch"]
    # value = committed / s over the timed steps: abort_rate ties it to ms_per_step (the line's
    # numbers carry 4 digits: abort_rate ~0.977 +- 5e-5 is +- 0.22 % of the committed share)
    assert rec["value"] == pytest.approx((1 - rec["abort_rate"]) * n_txn / (rec["ms_per_step"] * 1e-3), rel=5e-3)
    for k in ("roofline", "legs", "cpu_baseline", "detail"):
        assert k not in rec, k
    assert os.listdir(tmp_path) == ["out"]  # (no detail file, nothing else written)
    commit, st = np.load(tmp_path / "out" / "commit.npy"), np.load(tmp_path / "out" / "stats.npy")
    assert commit.dtype == np.float32 and commit.shape == (n_txn,) and set(np.unique(commit)) <= {0.0, 1.0}
    assert st[0] == n_txn and st[2] == commit.sum(dtype=np.float64) and st[2] + st[3] == n_txn and st[2] > 0
    f0 = np.load(tmp_path / "out" / "table_f0.npy")
    assert f0.dtype == np.float64 and f0.shape == (len(np.load(tmp_path / "out" / "table_rows.npy")), 2)


def test_synthetic_multi_gpu_record():
    kern = [{"kernel": f"k_{i}", "avg_us": 1.0 * i, "share": 0.01, "bytes": "x" * 300} for i in range(60)]
    out = {"metric": bench.METRIC, "value": 1.5e9, "unit": "committed txns/s", "n_gpus": 8, "steps": 20,
           "warmup": 5, "ms_per_step": 0.7, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "u64", "data": "synthetic", "config": {"workload": "w", "parallelism": "partitioned x8",
                                                            "sequence_order": "p" * 500},
           "roofline": {"kernel": "k_round_async", "bound": "hbm", "achieved": 30.0, "peak": 8000.0,
                        "unit": "GB/s", "frac": 0.004, "traffic": None, "bytes_per_launch": 1.5e6,
                        "avg_launch_ms": 0.05, "launches_per_epoch": 2.0, "share_of_epoch": 0.3,
                        "timed_by": "z" * 400, "algorithmic_bytes": "y" * 400},
           "cpu_baseline": {"value": 2e6, "unit": "committed txns/s", "cores": 16, "kind": "port",
                            "sample": "s" * 2000, "threads_scaling": {"1": 1e6, "4": 3e6, "16": 2e6}},
           "kernels": kern, "mpr_sweep": [{"mpr": m / 10, "committed_per_s": 1e9, "ms_per_step": 0.7,
                                           "abort_rate": 0.9, "steps": 10, "rounds_mean": 30.0}
                                          for m in range(6)],
           "strong_scaling": {"txns_per_epoch": 1 << 20, "ms_per_epoch": 0.5, "committed_per_s": 1e8},
           "tpcc_partitioned": {"warehouses": 256, "WAIT_DIE": {"txns_per_epoch": 65536, "ms_per_epoch": 0.3,
                                                                "committed_per_s": 1e6}}}
    rec = _check(bench.headline_record(out, "gpurun_out/bench_detail.json"), out)
    assert len(rec["legs"]["mpr_sweep"]) == 6 and "kernels" not in rec
    assert rec["legs"]["tpcc_partitioned"]["WAIT_DIE"]["ms_per_epoch"] == 0.3
