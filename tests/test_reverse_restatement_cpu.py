"""The host restatement that tests/test_gpu_reverse_index.py measures the reverse-index builder against (tests/reverse_restatement.py),
pinned on the CPU: its constants against the text of reverse.hip, its index on an example worked by hand, and -- the point of the case table
-- which case reaches which path of knn_reverse_kernel, so that the GPU file cannot silently test something else."""
import os
import re

import numpy as np
import pytest

import reverse_restatement as rr

REVERSE_HIP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mlsp_amd", "csrc", "reverse.hip")
_cache = {}


def _case(name, skip_pad):
    key = (name, bool(skip_pad))
    if key not in _cache:
        c = rr.CASES[name]
        idx = rr.case_idx(name)
        _cache[key] = (c, rr.reverse_paths(idx, c.N, skip_pad), rr.reverse_reference(idx, c.N, skip_pad))
    return _cache[key]


def test_constants_match_the_kernel_source():
    src = open(REVERSE_HIP).read()
    m = re.search(r"^#define RV_SPLIT_MAX (\d+)\b", src, re.M)
    assert m and int(m.group(1)) == rr.RV_SPLIT_MAX
    m = re.search(r"^#define RV_CAP \((\d+) \* (\d+)\)", src, re.M)
    assert m and int(m.group(1)) * int(m.group(2)) == rr.RV_CAP
    m = re.search(r"^\s*constexpr int RV_B = (\d+);", src, re.M)
    assert m and int(m.group(1)) == rr.RV_B
    # the block size and the launcher's slice rule, as the restatement states them
    assert "hipLaunchKernelGGL(knn_reverse_kernel, dim3(B * nsplit), dim3(%d)," % rr.RV_THREADS in src
    assert "const int nsplit = B * 8 >= 256 || N < 1024 ? 8 : RV_SPLIT_MAX;" in src
    assert "if (lds > 160 * 1024) return MLSP_ERR_UNSUPPORTED;" in src and rr.RV_LDS_LIMIT == 160 * 1024


def test_reference_on_a_hand_written_example():
    """B = 1, S = 2 groups of k = 3 over N = 4 points: group 0 = (2, 0, 2), group 1 = (1, 1, 2).
    Entries (i << 8) | s:  point 0 <- (0,1) = 1;  point 1 <- (1,0) = 256, (1,1) = 257;  point 2 <- (0,0) = 0, (0,2) = 2, (1,2) = 258;
    point 3 <- nothing.  With skip_pad a group's TRAILING repeats of its slot 0 go: (0,2).  (1,1) repeats slot 0 too, but slot (1,2) after
    it does not: an ordinary slot, which stays listed -- the consumer replaces the skipped slots by multiples of the group's LAST row, and
    the last row of group 1 belongs to point 2.  (Until the padding was defined as the trailing run, this example pinned (1,1) as skipped.)"""
    idx = np.array([[[2, 0, 2], [1, 1, 2]]], dtype=np.int32)
    r = rr.reverse_reference(idx, 4)
    assert r.rev_off.tolist() == [0, 1, 3, 6, 6]
    assert r.rev_ent.tolist() == [1, 256, 257, 0, 2, 258]
    assert r.listed.all() and r.rev_cnt.tolist() == [1, 2, 3, 0] and r.pad_cnt.tolist() == [0, 0]
    r = rr.reverse_reference(idx, 4, skip_pad=True)
    assert r.rev_off.tolist() == [0, 1, 3, 5, 6]
    assert r.rev_ent.tolist() == [1, 256, 257, 0, 258, -1]
    assert r.listed.tolist() == [True] * 5 + [False] and r.rev_cnt.tolist() == [1, 2, 2, 0] and r.pad_cnt.tolist() == [1, 0]
    # a second cloud starts at b * S * k whatever the first one left unfilled
    r = rr.reverse_reference(np.concatenate([idx, idx[:, ::-1]]), 4, skip_pad=True)
    assert r.rev_off.tolist() == [0, 1, 3, 5, 6, 7, 9, 11, 12]
    assert r.rev_ent.tolist() == [1, 256, 257, 0, 258, -1, 257, 0, 1, 2, 256, -1] and r.pad_cnt.tolist() == [1, 0, 0, 1]
    # a row that is one point throughout is slot 0 plus k - 1 padding slots; a lone repeat in the middle is not padding
    r = rr.reverse_reference(np.array([[[3, 3, 3], [3, 3, 0]]], dtype=np.int32), 4, skip_pad=True)
    assert r.pad_cnt.tolist() == [2, 0] and r.rev_cnt.tolist() == [1, 0, 0, 3]


def test_ball_like_groups():
    rng = np.random.default_rng(5)
    idx = rr.ball_like(rng, 2, 9, 40, 6)
    h = (idx != idx[:, :, :1]).sum(-1) + 1
    assert h[0, 0] == 1 and h[0, 1] == 6 and h.min() >= 1 and h.max() <= 6
    for g, hh in zip(idx.reshape(-1, 6), h.reshape(-1)):
        assert (np.diff(g[:hh]) > 0).all() and (g[hh:] == g[0]).all()
    hub = rr.with_hub(idx)
    assert (hub[:, :, 0] == 0).all() and ((hub != hub[:, :, :1]).sum(-1) + 1 == h).all()


@pytest.mark.parametrize("name", list(rr.CASES))
def test_case_reaches_its_path(name):
    c, slices, ref = _case(name, rr.CASES[name].skip_pad)
    assert len(slices) == c.B * slices[0].nsplit
    for n, pred in enumerate(c.path):
        assert pred(c, slices, ref), (name, n)
    # the figures that do not depend on the path: every kept slot is listed once, the lists tile the cloud's region from its start
    assert ref.rev_cnt.sum() == ref.listed.sum() == c.B * c.S * c.k - ref.pad_cnt.sum()
    assert sum(s.sn for s in slices) == ref.rev_cnt.sum()
    assert rr.reverse_lds_bytes(c.B, c.N)[2] <= rr.RV_LDS_LIMIT


@pytest.mark.parametrize("skip_pad", [False, True])
def test_every_path_is_reached(skip_pad):
    """Every case runs through the builder with and without skip_pad (tests/test_gpu_reverse_index.py): across all of their slices every
    value of every dispatch decision occurs, in either mode."""
    slices = [s for name in rr.CASES for s in _case(name, skip_pad)[1]]
    live = [s for s in slices if s.sn]
    assert {s.one_trip for s in live} == {True, False}
    assert {s.in_lds for s in live} == {True, False}
    assert {s.compacted for s in live if not s.one_trip and s.in_lds} == {True, False}
    assert {s.nsplit for s in slices} == {8, rr.RV_SPLIT_MAX}
    assert set().union(*(s.classes for s in live if s.in_lds)) == {rr.LE64, rr.MID, rr.BIG}
    assert any(s.nd == 0 for s in slices) and any(0 < s.nd < s.dper for s in slices)
    if skip_pad:
        # the fill that scans idx again has padding slots to leave out a second time, ordering in LDS and in global memory
        rescans = [s for s in live if not s.one_trip and not s.compacted and s.skipped > 0]
        assert {s.in_lds for s in rescans} == {True, False}
        assert any(s.skipped > 0 for s in live if s.one_trip) and any(s.skipped > 0 for s in live if s.compacted)


def test_unsupported_shape_of_the_error_path():
    """N = 50000 needs more LDS than the launcher allows (tests/test_gpu_reverse_index.py expects MLSP_ERR_UNSUPPORTED before any launch)"""
    assert rr.reverse_lds_bytes(1, 50000)[2] > rr.RV_LDS_LIMIT
