"""Which kernel a kNN search of a given shape runs on is decided by one host-only function (csrc/knn_plan.h) that launch_knn follows.
tools/knn_plan_host_check/main.cpp sweeps its invariants on the CPU and prints the plan of every shape it is given; here it is given
every shape the kNN tests search (tests/knn_shapes.py), and the kernel each one names is asserted -- a test comment about "the v4 path"
cannot drift from the dispatch again -- together with the coverage: every family / channel tile / v5 RES and KB variant the plan can
return is reached by a shape some test searches.  Built with whatever host compiler is at hand and plain flags."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import knn_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What functional.knn_graph gives the search: rows and planes on 16-byte boundaries (fresh tensors; the workspace carves at 256 bytes), and
# a workspace of mlsp_workspace_bytes(B N, C, 1), whose fixed term alone -- 32 MiB -- is left for the planes behind the norms.  (The
# workspace only grows, so a call may find more; no shape here needs more.)
PLANES_AT_HAND = 32 << 20


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = next((c for c in map(shutil.which, ("hipcc", "clang++", "g++")) if c), None)
    if cc is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("knn_plan")
    exe = str(tmp / "knn_plan_host_check")
    subprocess.run([cc, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "knn_plan_host_check", "main.cpp"), "-o", exe], check=True, cwd=str(tmp))

    def run(rows):
        """rows of (B, N, C, k, ld) -> (the labels of their plans, the labels the tool's sweep reached)"""
        text = "".join("%d %d %d %d %d 1 %d 1\n" % (tuple(r) + (PLANES_AT_HAND,)) for r in rows)
        r = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0 and "knn_plan_host_check: ok" in r.stdout, r.stdout[-4000:]
        plans = re.findall(r"^plan (\d+) (\d+) (\d+) (\d+) -> (\S+) lds \d+ grid \S+ block \d+ planes (\d+)", r.stdout, re.M)
        assert len(plans) == len(rows)
        assert all(int(p[5]) <= PLANES_AT_HAND for p in plans)
        return [p[4] for p in plans], set(re.findall(r"^reach (\S+)", r.stdout, re.M))
    return run


def _pins():
    """(where, B, N, C, k, ld, label) of every search of the kNN tests"""
    pins = [("test_knn_bit_exact_vs_oracle", B, N, C, k, C, label) for B, N, C, k, label in knn_shapes.BIT_EXACT]
    pins += [(name, *s) for name, shapes in knn_shapes.OTHER.items() for s in shapes]
    gdir = os.path.join(ROOT, "tests", "golden")
    names = sorted(f for f in os.listdir(gdir) if f.startswith("knn_"))
    assert names == sorted(knn_shapes.GOLDEN)
    for f in names:
        g = np.load(os.path.join(gdir, f))
        (B, C, N), k = g["x"].shape, g["idx"].shape[-1]
        pins.append(("golden " + f, B, N, C, k, C, knn_shapes.GOLDEN[f]))
    return pins


def test_the_workspace_leaves_the_planes_their_32_mib():
    src = open(os.path.join(ROOT, "mlsp_amd", "csrc", "api.hip")).read()
    body = src[src.index("size_t mlsp_workspace_bytes("):src.index("int mlsp_gemm_f32(")]
    assert re.search(r"return act \+ parts \+ wts \+ .*\(32 << 20\)", body)
    assert "r * sizeof(float)" in body                              # the norms that mlsp_knn_f32 takes in front of the planes


def test_every_knn_test_shape_reaches_the_kernel_it_names(check):
    pins = _pins()
    assert len({p[1:5] for p in pins if p[0] == "test_knn_bit_exact_vs_oracle"}) == len(knn_shapes.BIT_EXACT)        # no shape twice
    labels, _ = check([p[1:6] for p in pins])
    wrong = [(p[0], p[1:6], "named " + p[6], "plan " + got) for p, got in zip(pins, labels) if got != p[6]]
    assert not wrong, wrong


def test_every_kernel_variant_is_reached_by_a_test_shape(check):
    """Every label of the sweep (vector / scalar loads apart): family, channel tile, v5's RES and KB -- also of the v5 kernel behind the
    wide one -- and the VALU kernel's KMAX.  (KMAX = 20 is in no plan: k <= 20 goes to a matrix-core kernel for every C <= 256, and the VALU
    kernel's tiles do not hold C > 256.)"""
    _, reach = check([])
    assert len(reach) >= 30 and {"VEX", "V4/4", "V3/256", "VALU/40/c3", "V5/128/kb"} <= reach and not any("vec" in r for r in reach)
    pinned = {re.sub(r"vec,|[/,]vec$", "", p[6]) for p in _pins()}
    assert sorted(reach - pinned) == []
    assert sorted(pinned - reach) == []
