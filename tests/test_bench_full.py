"""bench.py --full: a plain run does only what its headline needs; the checks and further measurements (identity vs truth,
oracle parity samples, other configs, CPU baseline) run only with --full, after the timed region."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_full_is_opt_in():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True
    a = bench.parse_args(["--full", "--no-cpu", "--other-configs", "none", "--cpu-seconds", "2"])
    assert a.no_cpu and a.other_configs == "none" and a.cpu_seconds == 2.0


def _run(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reads", "512", "--steps", "2", "--warmup", "1"] + list(extra)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    out = json.loads(lines[0])
    assert all(k in out for k in HEADLINE)
    assert out["metric"] == "R2C2 reads->consensus/sec" and out["unit"] == "reads/s" and out["higher_is_better"] is True
    assert out["value"] == pytest.approx(512 * out["steps"] / (out["ms_per_step"] * out["steps"] * 1e-3), rel=1e-3)
    return out


@pytest.mark.gpu
def test_plain_run_has_no_extras():
    out = _run()
    assert out["steps"] == 2 and out["warmup"] == 1
    for k in ("parity_sample", "other_configs", "cpu_baseline"):
        assert k not in out, k
    assert "identity_vs_truth" not in out["config"] and out["config"]["consensus_ok"] >= 510
    assert out["roofline"]["kernel"].startswith("k_")


@pytest.mark.gpu
def test_full_run_has_every_check():
    out = _run("--full", "--other-configs", "cfg1", "--cpu-seconds", "1")
    assert out["parity_sample"]["reads"] == 64 and out["parity_sample"]["mismatches"] == 0
    assert out["config"]["identity_vs_truth"]["reads"] == 200 and out["config"]["identity_vs_truth"]["mean"] > 0.9
    o = out["other_configs"]["cfg1"]
    assert o["reads_per_step"] == bench.DEFAULT_READS["cfg1"] and o["value"] > 0 and o["parity_sample"]["mismatches"] == 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["kind"] == "port"
