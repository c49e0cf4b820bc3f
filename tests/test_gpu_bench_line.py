"""GPU: the line bench.py prints.  A plain run carries the headline and none of the side measurements, which take runs of
their own; --full adds them (checked here with `roofline`, the one the tools/ scripts read: the others take minutes)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 300                               # seconds for one bench.py child run
NB = 6144                                   # bench.py's T30 batch per GPU
SIDE = ("roofline", "multi_gpu", "extras", "cpu_baseline", "cpu_baseline_fast_math", "cpu_baseline_socket",
        "gpu_over_cpu_core", "gpu_over_cpu_socket")


def bench_line(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "2"] + list(args)
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=TIMEOUT)
    assert run.returncode == 0, "bench.py exited with status %d\n%s" % (run.returncode, run.stderr[-3000:])
    lines = run.stdout.strip().splitlines()
    assert lines, run.stderr[-3000:]
    return json.loads(lines[-1])


def test_plain_line_is_the_headline():
    line = bench_line()
    assert line["metric"] == "spectral transforms/sec (grid<->spec round-trip) at T30 L8"
    assert line["unit"] == "round trips/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["value"] > 0 and line["steps"] == 20 and line["warmup"] == 2
    # value = fields x steps / median block, ms_per_step = median block / steps
    assert line["ms_per_step"] * line["value"] == pytest.approx(1e3 * NB, rel=1e-9)
    assert [k for k in SIDE if k in line] == []
    assert line["errors"] == []


def test_full_line_adds_the_side_measurements():
    line = bench_line("--full", "--no-extras", "--no-cpu-baseline", "--no-pmc")
    assert line["value"] > 0
    rf = line["roofline"]
    assert rf["kernel"] in rf["all_kernels_ms"] and rf["launch_ms"] > 0 and rf["frac"] > 0
    assert "extras" not in line and "cpu_baseline" not in line
    assert line["errors"] == []
