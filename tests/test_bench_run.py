"""bench.py run end to end on a small C3-shaped workload: a plain run prints the headline and what its timed region
measured, and leaves what takes runs of its own (the per-kernel breakdown pass, the CPU baseline, the secondary
lines) to --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "16", "--warmup", "4", "--ids", "2000000", "--rows", "2000", "--distinct", "8"]


def test_full_is_off_by_default(monkeypatch):
    # (bench.py sets this variable on import when it is unset: the test leaves the environment as it found it)
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2"])
    assert bench.parse_args().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse_args().full is True


def run_bench(extra):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "bench.py")] + SMALL + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def check_headline(d):
    for k, typ in dict(metric=str, value=float, unit=str, higher_is_better=bool, dtype=str, ms_per_step=float).items():
        assert isinstance(d[k], typ), k
    assert d["steps"] == 16 and d["warmup"] == 4 and d["unit"] == "examples/sec" and d["dtype"] == "f32"
    assert abs(d["value"] - 2000 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    # the live HIP events ride inside the timed region in both kinds of run
    assert d["roofline"]["launches_timed"] > 0 and d["roofline_backward"]["launches_timed"] > 0


@pytest.mark.gpu
def test_plain_run_leaves_the_extras_to_full():
    d = run_bench([])
    check_headline(d)
    assert d["full"] is False
    assert d["kernel_ms_per_step"] == {} and d["cpu_baseline"] is None and d["secondary"] is None

    f = run_bench(["--full", "--no-secondary", "--cpu-batches", "2"])
    check_headline(f)
    assert f["full"] is True and f["secondary"] is None
    assert {"forward", "backward"} <= set(f["kernel_ms_per_step"])
    c = f["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["value"] > 0 and c["unit"] == "examples/sec"
