"""bench.py on the GPU, on a small box: a plain run prints the headline and measures nothing outside its timed steps;
--full adds the pair count, the pass that times the dominant kernel with its roofline and the secondary legs."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
BEYOND_HEADLINE = ("pairs_in_cutoff", "pair_interactions_per_s", "roofline", "secondary", "cpu_baseline")


def _bench(*args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nside", "12", "--steps", "20",
                          "--warmup", "5", "--relax-steps", "50", *args], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def test_bench_plain_and_full_lines(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path))
    full = _bench("--full", "--no-cpu-baseline")
    for d in (plain, full):
        assert all(k in d for k in HEADLINE)
        assert d["unit"] == "ns/day" and d["higher_is_better"] is True and d["dtype"] == "f32"
        assert d["steps"] == 20 and d["warmup"] == 5 and d["value"] > 0
        assert abs(d["value"] * d["ms_per_step"] - 86.4) < 1e-9 * 86.4  # ns/day of 1-fs steps at ms_per_step
        assert d["list"]["algorithm"] == "celllist"
    assert plain["metric"] == full["metric"] and plain["config"] == full["config"]
    assert not set(BEYOND_HEADLINE) & set(plain)
    assert sorted(plain["outputs"]["arrays"]) == ["ekin", "epot", "forces", "pos", "temperature", "vel"]
    assert all(os.path.exists(tmp_path / f"{n}.npy") for n in plain["outputs"]["arrays"])
    assert full["pairs_in_cutoff"] > 0 and full["roofline"]["bound"] == "hbm" and "avg_kernel_us" in full["roofline"]
    assert full["secondary"]["c3_switch"]["value"] > 0 and "cpu_baseline" not in full
