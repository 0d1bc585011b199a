"""What a GEMM launch of a given shape does -- kernel family, split-K count, tile height, grid, status -- is decided by one host-only
function (csrc/gemm_plan.h) that the launcher follows and the shape queries are statements over.  tools/gemm_plan_host_check/main.cpp
sweeps it on the CPU: the queries against the plan over a grid of shapes, the plans of every GEMM launch of a configs[1] and a configs[4]
step as listed on the MI355X before the plan existed, and the folded / N = 64 corners; with whatever host compiler is at hand and plain flags."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gemm_plan_host_check(tmp_path):
    cc = next((c for c in map(shutil.which, ("hipcc", "clang++", "g++")) if c), None)
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "gemm_plan_host_check")
    subprocess.run([cc, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "gemm_plan_host_check", "main.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "gemm_plan_host_check: ok" in r.stdout, r.stdout
