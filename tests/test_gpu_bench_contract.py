"""bench.py is the driver's measurement contract: one JSON line on stdout with the agreed keys, whatever else changes.
Runs the real script (tiny K / W) on the GPU and checks the line: with --full (roofline and the step without dropout; the
extras and the CPU baseline off), and plain, where it also writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_keys():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--kernel-reps", "1",
                        "--no-cpu-baseline", "--no-extras", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["unit"] == "quadruplets/s" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "bf16" and d["data"] == "synthetic"
    assert abs(d["value"] - 64 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]              # whole-job throughput = B / step time
    cfg = d["config"]
    assert "workload" in cfg and "dropout 0.1" in cfg["workload"] and "model" not in cfg
    assert cfg["global_batch"] == 64 and cfg["seq_len"] == 128 and cfg["parallelism"] == "dp1"
    ro = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "hbm_side"):
        assert k in ro, k
    assert ro["bound"] in ("hbm", "mfma") and abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-3
    assert d["step_without_dropout"]["value"] >= d["value"] * 0.9


def test_plain_run_times_the_headline_step_and_dumps_its_outputs(tmp_path):
    import numpy as np
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "loss"):
        assert k in d, k
    assert d["unit"] == "quadruplets/s" and d["dtype"] == "bf16" and d["steps"] == 4 and d["warmup"] == 2
    assert abs(d["value"] - 64 / (d["ms_per_step"] * 1e-3)) < 0.01 * d["value"]
    for k in ("step_without_dropout", "roofline", "fwd_only", "golden_parity", "cpu_baseline"):        # --full only
        assert k not in d, k
    names = sorted(os.listdir(tmp_path))
    assert names == ["grad_norm.npy", "loss.npy", "params.npy"], names
    assert sum(os.path.getsize(tmp_path / n) for n in names) <= 64 << 20
    a = {n[:-4]: np.load(tmp_path / n) for n in names}
    assert all(x.dtype in (np.float32, np.float64) and np.isfinite(x).all() for x in a.values())
    assert abs(float(a["loss"][0]) - d["loss"]) < 1e-5 and a["grad_norm"][0] > 0
    assert a["params"].shape == (1 << 21,) and np.abs(a["params"]).max() > 0       # MiniLM's arena (22.7M) is sampled
