"""bench.py on the GPU: a plain run prints the headline line and measures nothing else; --full adds the profiled / counted figures
after the timed steps (the parts skipped by --no-cpu-baseline / --no-secondary / --no-fp32-leg are left out here to keep the test short)."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "blocks_ms_per_step"}
FULL_ONLY = {"roofline", "roofline_kernels", "executed_tflops", "launches_source", "fp32_mfma", "bf16x6_split", "distributed",
             "secondary", "cpu_baseline"}


def _bench(args):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only(tmp_path):
    out = _bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "d")])
    assert HEADLINE <= set(out) and not FULL_ONLY & set(out), sorted(out)
    assert out["full"] is False and out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "points/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert abs(out["value"] - 32 * 1024 / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    assert out["dump_outputs"]["arrays"] == len(os.listdir(str(tmp_path / "d"))) > 0


def test_full_run_adds_the_profiled_figures():
    out = _bench(["--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-secondary", "--no-fp32-leg"])
    assert HEADLINE <= set(out) and out["full"] is True
    assert {"roofline", "roofline_kernels", "executed_tflops", "launches_source"} <= set(out), sorted(out)
    assert not {"secondary", "cpu_baseline", "fp32_mfma", "bf16x6_split", "distributed"} & set(out), sorted(out)
    assert out["roofline"]["achieved"] > 0
