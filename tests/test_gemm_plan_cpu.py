"""What a GEMM launch of a given shape does -- kernel family, split-K count, tile height, grid, status, the kernel that sums the slabs -- is
decided by host-only functions (csrc/gemm_plan.h) that the launcher follows and the shape queries are statements over.
tools/gemm_plan_host_check/main.cpp sweeps them on the CPU: the queries against the plan over a grid of shapes, the plans of every GEMM
launch of a configs[1] and a configs[4] step as listed on the MI355X before the plan existed, and the folded / N = 64 corners; and it
prints the plan of every launch it is given.  Here it is given every launch the GEMM tests make (tests/gemm_shapes.py), and the kernel
each row names is asserted -- a comment about "both tile heights, split-K" cannot drift from gemm_pick_split / gemm_pick_bm /
gemm_split_pays again -- together with the coverage: every label the tool's sweep reaches is pinned by some row.  With whatever host
compiler is at hand and plain flags."""
import os
import re
import shutil
import subprocess

import pytest

import gemm_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cc = next((c for c in map(shutil.which, ("hipcc", "clang++", "g++")) if c), None)
    if cc is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("gemm_plan")
    exe = str(tmp / "gemm_plan_host_check")
    subprocess.run([cc, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "gemm_plan_host_check", "main.cpp"), "-o", exe], check=True, cwd=str(tmp))

    done = {}

    def run(rows):
        """rows of gemm_shapes.Row -> ([(label, (grid_x, grid_y), reducer)] of their plans, the labels the tool's sweep reached, its output,
        its exit status).  What functional.gemm gives the launch: the slab the shape asks for, C and the slab on 16-byte boundaries."""
        if tuple(rows) in done:                                                 # (the sweep is the same every time: one run per question)
            return done[tuple(rows)]
        text = ""
        for r in rows:
            text += "%d %d %d %d %d %d %d %d %d " % ((gemm_shapes.MODES[r.mode], r.ta, r.tb, r.M, r.N, r.K) + gemm_shapes.pitches(r))
            text += "%d %d %d 1 %d -1\n" % (r.off[0] == 0, r.off[1] == 0, r.bias != 0, r.bias != 2)
        p = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert "gemm_plan_host_check: " in p.stdout, p.stdout[-4000:]           # (ran to its end; its own verdict: test_gemm_plan_host_check)
        plans = re.findall(r"^plan \d \d \d \d+ \d+ \d+ -> (\S+) grid (\d+),(\d+) vec \d\d reduce (\S+)$", p.stdout, re.M)
        assert len(plans) == len(rows)
        done[tuple(rows)] = ([(l, (int(x), int(y)), red) for l, x, y, red in plans], set(re.findall(r"^reach p\d:(\S+) <- ", p.stdout, re.M)), p.stdout,
                             p.returncode)
        return done[tuple(rows)]
    return run


def test_gemm_plan_host_check(check):
    _, reach, out, rc = check([])
    assert rc == 0 and "agreement:" in out and "gemm_plan_host_check: ok" in out and "FAILED" not in out, out[-4000:]
    assert len(reach) >= 40


def _any_ns(label):
    """the label with its number of splits set aside: ns=1 or ns>1"""
    return re.sub(r"ns=(\d+)", lambda m: "ns=1" if m.group(1) == "1" else "ns>1", label)


def test_every_gemm_test_launch_reaches_the_kernel_it_names(check):
    named = gemm_shapes.rows()
    assert len(named) == len(set(named))                                        # no launch twice in one test
    plans, _, _, _ = check([r for _, r in named])
    wrong = []
    for (name, r), (label, grid, red) in zip(named, plans):
        if label != r.label:
            wrong.append((name, r[:6], "named " + r.label, "plan " + label))
        if r.via in ("tile", "fold"):
            if red != r.reduce:
                wrong.append((name, r[:6], "reducer named " + r.reduce, "plan " + red))
            if grid != gemm_shapes.grid(r) and r.via == "tile":
                wrong.append((name, r[:6], "grid %r" % (gemm_shapes.grid(r),), "plan %r" % (grid,)))
        else:
            assert r.reduce == "-" and ("thin?" if r.via == "thin" else "skinny?") in r.label, (name, r)
        assert (r.via == "fold") == r.label.startswith("FOLD64:"), (name, r)
    assert not wrong, wrong


def test_every_kernel_variant_is_reached_by_a_test_launch(check):
    """Every label the sweep reaches for plain and bias launches through mlsp_gemm_f32 -- family, tile height, one pass or split-K, xcd_map,
    interior tiles, f16 pieces or eligible and kept on six products, the offers -- is pinned by some row, and the other way round; the
    number of splits apart (the load widths are not in a label: ragged and pitched rows take the scalar loads).  The launch options of
    the layers (gemm_shapes' docstring) are not part of it."""
    _, reach, _, _ = check([])
    reach = {_any_ns(l) for l in reach}
    pinned = {_any_ns(r.label) for _, r in gemm_shapes.rows()}
    assert sorted(reach - pinned) == []
    assert sorted(pinned - reach) == []
    # ... and by a row that the tile kernel really runs, where anything can make it run (an offer that is always taken hides the kernel)
    ran = {_any_ns(r.label) for _, r in gemm_shapes.rows() if r.via in ("tile", "fold")}
    assert sorted(reach - ran) == []


def test_every_reducer_and_every_layout_is_pinned():
    tile = [r for _, r in gemm_shapes.rows() if r.via == "tile"]
    assert {r.reduce for r in tile} == {"-", "VEC8", "VEC4", "VEC1", "WAVE", "SCALAR"}
    assert {r.reduce for r in tile if r.bias} >= {"VEC8", "VEC4", "VEC1", "WAVE", "SCALAR"}      # a bias under split-K is the reducer's
    layouts = {}
    for r in tile:
        fam = gemm_shapes.parse(r.label)[0]
        layouts.setdefault(fam, set()).add((r.ta, r.tb))
        if "/pieces/" in r.label:
            layouts.setdefault("f16 pieces, bm %d" % gemm_shapes.parse(r.label)[1], set()).add((r.ta, r.tb))
            if gemm_shapes.parse(r.label)[2] > 1:
                layouts.setdefault("f16 pieces, split-K", set()).add((r.ta, r.tb))
            if gemm_shapes.parse(r.label)[3] == 0:
                layouts.setdefault("f16 pieces, no XCD map", set()).add((r.ta, r.tb))
    every = {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert set(layouts) == {"N64", "F32_EDGE", "F32", "BF16", "SPLIT", "f16 pieces, bm 128", "f16 pieces, bm 64", "f16 pieces, split-K",
                            "f16 pieces, no XCD map"}
    for fam, seen in layouts.items():
        assert seen == (every - {(1, 1)} if fam == "N64" else every), (fam, seen)       # (the 64-column kernel has no A^T B^T)
    # the addressing cases: pitches dim + 1 and dim + 4 on every operand and on C, A and B 4 bytes off, both kinds of bias, also under split-K
    assert {p for r in tile for p in r.pad} >= {0, 1, 4} and all({r.pad[i] for r in tile} >= {0, 1, 4} for i in range(3))
    assert {r.off for r in tile} >= {(0, 0), (1, 0), (0, 1)}
    for via in ("thin", "skinny"):                                              # the offers behind pitched and offset operands and a pitched C
        assert any(r.via == via and r.off != (0, 0) and all(r.pad) for _, r in gemm_shapes.rows()), via
    pieces = {gemm_shapes.parse(r.label)[1:] for r in gemm_shapes.PIECE_TIER if "/pieces/" in r.label}
    assert {(bm, ns > 1, xcd) for bm, ns, xcd in pieces} >= {(128, False, 0), (128, True, 0), (128, False, 1), (128, True, 1), (128, True, 2), (64, False, 0), (64, False, 1)}
    assert {r.bias for r in tile if r.reduce != "-"} == {0, 1, 2} and {r.bias for r in tile if r.reduce == "-"} == {0, 1, 2}
    assert len(gemm_shapes.PIECE_TIER) >= 16 and {r.mode for r in gemm_shapes.PIECE_TIER} == {"bf16x6", "f16x3"}
