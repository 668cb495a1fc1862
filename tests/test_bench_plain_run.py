"""bench.py without --full on the CPU: the device layer is the double of test_bench_eight_ranks (answers from the committed
oracle golden). A plain run makes the cold pass, --warmup and --steps steps and nothing else, prints one headline line and
writes no record file; --dump-outputs writes what the last timed step returned."""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

from test_bench_eight_ranks import FakeBatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class CountingBatch(FakeBatch):
    """FakeBatch that counts its launches; a step takes at least STEP_S."""
    launches = None
    STEP_S = 0.002

    def generate_poa(self):
        CountingBatch.launches["generate_poa"] += 1
        time.sleep(CountingBatch.STEP_S)

    def relaunch(self):
        CountingBatch.launches["relaunch"] += 1

    def relaunch_timed(self):
        CountingBatch.launches["relaunch"] += 1
        return 1.0, 0.1


def _run(monkeypatch, argv):
    import torch
    import golden_io
    from genomeworks_amd import cuda, cudapoa, synthetic
    rows, _ = golden_io.config3_windows()
    FakeBatch.rows = rows
    FakeBatch.by_first_read = {synthetic.generate_window(1000 + w)[0].decode(): w for w in range(len(rows))}
    CountingBatch.launches = {"generate_poa": 0, "relaunch": 0}
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "GW_BENCH_RANKS_PER_DEVICE"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(cudapoa, "CudaPoaBatch", CountingBatch)
    monkeypatch.setattr(cuda, "cuda_set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main()
    return buf.getvalue(), rows


def test_plain_run_times_the_steps_and_prints_the_headline_only(monkeypatch, tmp_path):
    record = tmp_path / "record"
    dump = tmp_path / "dump"
    out, rows = _run(monkeypatch, ["--gpus", "1", "--steps", "3", "--warmup", "2", "--record-dir", str(record),
                                   "--dump-outputs", str(dump)])
    lines = out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus", "config"):
        assert key in line, key
    assert line["unit"] == "GCUPS" and line["dtype"] == "int16" and line["higher_is_better"] is True
    assert line["steps"] == 3 and line["warmup"] == 2 and line["value"] > 0
    assert line["ms_per_step"] >= CountingBatch.STEP_S * 1e3
    assert line["config"]["cells_per_gpu"] == 10990578176
    for key in ("sub_records", "roofline", "cpu_baseline", "equals_oracle_golden", "kernel_only"):
        assert key not in line, key
    # the cold pass, the warm-up and the timed steps: no other launch
    assert CountingBatch.launches == {"generate_poa": 1 + 2 + 3, "relaunch": 0}
    assert not record.exists()
    # what the last step returned, window by window
    got = {p[:-4]: np.load(dump / p) for p in os.listdir(dump)}
    assert set(got) == {"consensus", "coverage", "consensus_length", "status", "window"}
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(os.path.getsize(dump / (k + ".npy")) for k in got) <= 64 << 20
    assert got["consensus"].shape[0] == len(rows) and (got["window"] == np.arange(len(rows))).all()
    for w in (0, 1, 511, len(rows) - 1):
        n = int(got["consensus_length"][w])
        assert got["consensus"][w, :n].astype(np.uint8).tobytes().decode() == rows[w]["consensus"]
        assert (got["consensus"][w, n:] == 0).all()
        assert got["coverage"][w, :n].tolist() == list(rows[w]["coverage"])
        assert got["status"][w] == rows[w]["status"]


def test_full_run_keeps_the_checks_and_the_record(monkeypatch, tmp_path):
    out, _ = _run(monkeypatch, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline",
                                "--sub-configs", "none", "--record-dir", str(tmp_path)])
    line = json.loads(out.strip().splitlines()[-1])
    assert line["equals_oracle_golden"] is True and line["roofline"]["bound"] == "hbm" and "kernel_only" in line
    assert CountingBatch.launches["relaunch"] > 0
    assert (tmp_path / "bench_full_record.json").exists()


def test_dump_samples_large_outputs_with_a_fixed_seed(monkeypatch, tmp_path):
    import bench
    cons = ["ACGT" * (1 + w % 7) for w in range(200)]
    cov = [[w % 5 + 1] * len(c) for w, c in enumerate(cons)]
    monkeypatch.setattr(bench, "DUMP_LIMIT", 40 * 4 * (2 * 28 + 3))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), cons, cov, [0] * len(cons))
    win = np.load(tmp_path / "a" / "window.npy")
    assert len(win) == 40 and (np.diff(win) > 0).all()
    for name in ("window", "consensus", "coverage"):
        assert (np.load(tmp_path / "a" / (name + ".npy")) == np.load(tmp_path / "b" / (name + ".npy"))).all()
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT + 5 * 128  # (+ the .npy headers)
    c = np.load(tmp_path / "a" / "consensus.npy")
    w0 = int(win[0])
    assert c[0, :len(cons[w0])].astype(np.uint8).tobytes().decode() == cons[w0]
