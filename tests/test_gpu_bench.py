"""bench.py's command line on a device, at a small odd batch (300 sets: not a
multiple of any tile, several blocks): a plain run prints the headline line
only, --full adds the other legs' keys to the same line, and two plain runs
with --dump-outputs write identical files (seeded workload and randomizers).
Each run is a fresh child process, as the benchmark is run."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS, STEPS, WARMUP = 300, 3, 1
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "serial_stages", "workload_gen_s"}
FULL_ONLY_KEYS = {"value_1m", "config5_1m", "value_key_table", "ms_per_step_key_table", "key_table", "p50_latency_ms_128", "p99_latency_ms_128",
                  "latency_reps_128", "stage_ms_overlapped", "stage_ms_exclusive", "roofline", "configs", "kzg", "cpu_baseline"}


def run_bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                        "--sets-per-gpu", str(SETS), *extra], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def check_headline(line):
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["n_gpus"] == 1
    assert line["unit"] == "sigs/s" and line["higher_is_better"] is True and line["config"]["sets_per_gpu"] == SETS
    assert line["ms_per_step"] > 0
    # value is the sets of the STEPS timed steps over their time
    assert line["value"] == pytest.approx(SETS / (line["ms_per_step"] * 1e-3), rel=1e-9)


def test_plain_runs_print_the_headline_only_and_dump_identical_outputs(tmp_path):
    dumps = []
    for name in ("a", "b"):
        line = run_bench("--dump-outputs", str(tmp_path / name))
        assert set(line) == PLAIN_KEYS
        check_headline(line)
        dumps.append({f: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))})
    a, b = dumps
    assert sorted(a) == sorted(b) == ["partial_fp12.npy", "partial_invalid_sets.npy", "verdict.npy"]
    for f in a:
        assert a[f].dtype == np.float32 and np.array_equal(a[f], b[f]), f
    assert a["partial_fp12.npy"].shape == (1, 12, 48) and a["partial_fp12.npy"].max() <= 255 and a["partial_fp12.npy"].any()
    assert a["partial_invalid_sets.npy"].tolist() == [0.0] and a["verdict.npy"].tolist() == [1.0]


def test_full_line_holds_the_plain_keys_and_the_moved_ones():
    # the long legs trimmed by their own options; their keys stay in the line
    line = run_bench("--full", "--no-1m", "--no-extra", "--no-kzg", "--no-cpu-baseline", "--lat-reps", "5")
    assert set(line) == PLAIN_KEYS | FULL_ONLY_KEYS
    check_headline(line)
    assert line["latency_reps_128"] == 5 and line["p50_latency_ms_128"] > 0
    assert line["value_key_table"] > 0 and set(line["stage_ms_exclusive"]) == set(line["stage_ms_overlapped"])
    assert line["roofline"]["kernel_ms"] > 0
