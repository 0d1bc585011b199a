"""The per-call context of the GEMM family (csrc/callctx.h) is host-only code: tools/callctx_host_check/main.cpp runs its bookkeeping -- the
slot ring in the workspace tail, the measured-operand cache, the caller's bounds table, the one pending slot -- against heap buffers, with
whatever host compiler is at hand and plain flags."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_callctx_host_check(tmp_path):
    cc = next((c for c in map(shutil.which, ("hipcc", "clang++", "g++")) if c), None)
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "callctx_host_check")
    subprocess.run([cc, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "callctx_host_check", "main.cpp"), "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "callctx_host_check: ok" in r.stdout, r.stdout
