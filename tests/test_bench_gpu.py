"""GPU: what a plain `bench.py` run measures and what `--full` adds (small configuration, level 3 batch 8)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*flags):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "4", "--level", "3",
           "--batch", "8", *flags]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_other_records():
    plain = _bench()
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert key in plain, key
    assert plain["steps"] == 5 and plain["warmup"] == 4 and plain["value"] > 0
    assert abs(plain["value"] - 8 / (plain["ms_per_step"] * 1e-3)) <= 1e-6 * plain["value"]
    assert plain["roofline"]["frac"] > 0 and "dominant_kernel" not in plain["roofline"]
    assert "secondary" not in plain and "cpu_baseline" not in plain
    full = _bench("--full", "--no-extra", "--cpu-batch", "8")
    assert full["roofline"]["dominant_kernel"]["ms"] > 0
    assert full["secondary"]["images_per_s"] > 0
    assert full["cpu_baseline"]["value"] > 0
