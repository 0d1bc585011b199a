"""The reverse neighbour index (mlsp_amd/csrc/reverse.hip: knn_reverse_kernel, launch_reverse, group_pad_count_kernel) restated in plain numpy:
the exact index a host sort gives, the launcher's and the kernel's dispatch arithmetic (which slice of which cloud takes which path), a
builder of groups shaped like ball-query output, and the case table of tests/test_gpu_reverse_index.py.
Shared by tests/test_gpu_reverse_index.py and tests/test_reverse_restatement_cpu.py (which proves which case reaches which path)."""
import collections

import numpy as np

# restated from reverse.hip; tests/test_reverse_restatement_cpu.py reads the three lines there and fails when they drift
RV_CAP = 16 * 1024          # LDS entries of a slice's lists (a slice past that orders in place in global memory)
RV_B = 20                   # index loads in flight per thread: E <= RV_THREADS * RV_B entries is ONE trip
RV_SPLIT_MAX = 16           # workgroups per cloud: 8, or 16
RV_THREADS = 1024           # threads per workgroup (the launch's block size)
RV_LDS_LIMIT = 160 * 1024   # bytes: above it the launcher returns MLSP_ERR_UNSUPPORTED

LE64, MID, BIG = "<=64", "65..512", ">512"          # the list-length classes of the LDS ordering

Reverse = collections.namedtuple("Reverse", "rev_off rev_ent listed rev_cnt pad_cnt")
SlicePath = collections.namedtuple("SlicePath", "b part nsplit dper nd one_trip sn padded in_lds compacted classes longest skipped")


def _keep(idx, skip_pad):
    """[B][S][k] bool: the slots the lists hold (skip_pad: not the group's padding -- its TRAILING run of slots s > 0 that repeat slot 0,
    what a ball query appends; a repeat of slot 0 further up a row is an ordinary slot)"""
    keep = np.ones(idx.shape, dtype=bool)
    if skip_pad:
        differs = idx[:, :, 1:] != idx[:, :, :1]
        # a slot is kept iff it, or some slot after it, differs from slot 0
        keep[:, :, 1:] = np.flip(np.logical_or.accumulate(np.flip(differs, -1), -1), -1)
    return keep


def reverse_reference(idx, N, skip_pad=False):
    """The exact reverse index of idx [B][S][k] (values in [0, N)): per cloud and destination j the entries (i << 8) | s with
    idx[b][i][s] == j, ascending; skip_pad leaves out every group's trailing run of slots s > 0 whose index equals its slot 0.
    -> Reverse(rev_off [B*N+1] (a cloud's lists start at b*S*k; rev_off[B*N] = B*S*k), rev_ent [B*S*k] (-1 where no list lies),
    listed [B*S*k] bool (the positions that belong to a list), rev_cnt [B*N] list lengths, pad_cnt [B*S] skipped slots per group)."""
    idx = np.asarray(idx)
    B, S, k = idx.shape
    assert k <= 256 and idx.min() >= 0 and idx.max() < N
    E = S * k
    keep = _keep(idx, skip_pad)
    packed = ((np.arange(S, dtype=np.int64)[:, None] << 8) | np.arange(k, dtype=np.int64)[None, :]).reshape(-1)
    rev_off = np.empty(B * N + 1, dtype=np.int32)
    rev_ent = np.full(B * E, -1, dtype=np.int32)
    listed = np.zeros(B * E, dtype=bool)
    rev_cnt = np.empty(B * N, dtype=np.int32)
    for b in range(B):
        kb = keep[b].reshape(-1)
        j = idx[b].reshape(-1).astype(np.int64)[kb]
        p = packed[kb]
        order = np.argsort(j * (1 << 32) + p, kind="stable")        # by destination, then by (i, slot): the keys are distinct
        cnt = np.bincount(j, minlength=N)
        rev_cnt[b * N:(b + 1) * N] = cnt
        rev_off[b * N:(b + 1) * N] = b * E + np.cumsum(cnt) - cnt
        rev_ent[b * E:b * E + p.size] = p[order]
        listed[b * E:b * E + p.size] = True
    rev_off[B * N] = B * E
    pad_cnt = (~keep).sum(-1).reshape(-1).astype(np.int32)
    return Reverse(rev_off, rev_ent, listed, rev_cnt, pad_cnt)


def reverse_lds_bytes(B, N):
    """launch_reverse: (slices per cloud, destinations per slice, dynamic LDS bytes)"""
    nsplit = 8 if (B * 8 >= 256 or N < 1024) else RV_SPLIT_MAX
    dper = (N + nsplit - 1) // nsplit
    return nsplit, dper, (((3 * dper + 2 + 3) & ~3) + 2 * RV_CAP) * 4


def reverse_paths(idx, N, skip_pad):
    """The dispatch of launch_reverse / knn_reverse_kernel for idx [B][S][k], one SlicePath per (cloud, slice):
    nsplit, dper, nd (destinations of the slice: the last may be ragged, a slice past N is empty), one_trip (the cloud's S*k indices fit
    the registers of one pass), sn (entries of the slice's lists), padded (the same with every list padded to a multiple of 4: what the
    LDS image holds), in_lds (padded <= RV_CAP: ordered in LDS, otherwise in place in global memory), compacted (several trips, in LDS,
    and the slice's sn pairs fit RV_CAP / 2: the fill walks the pairs instead of scanning idx again), classes (the list-length classes
    among the slice's non-empty lists), longest, skipped (padding slots that point into the slice: what a rescanning fill must re-check)."""
    idx = np.asarray(idx)
    B, S, k = idx.shape
    nsplit, dper, lds = reverse_lds_bytes(B, N)
    assert lds <= RV_LDS_LIMIT
    E = S * k
    one_trip = E <= RV_THREADS * RV_B
    keep = _keep(idx, skip_pad)
    out = []
    for b in range(B):
        flat, kb = idx[b].reshape(-1), keep[b].reshape(-1)
        cnt = np.bincount(flat[kb], minlength=N)
        pads = np.bincount(flat[~kb], minlength=N)
        for part in range(nsplit):
            d0 = min(N, part * dper)
            d1 = min(N, d0 + dper)
            c = cnt[d0:d1]
            sn, padded = int(c.sum()), int(((c + 3) & ~3).sum())
            in_lds = padded <= RV_CAP
            compacted = (not one_trip) and in_lds and sn <= RV_CAP // 2
            classes = set()
            if ((c >= 1) & (c <= 64)).any():
                classes.add(LE64)
            if ((c > 64) & (c <= 512)).any():
                classes.add(MID)
            if (c > 512).any():
                classes.add(BIG)
            out.append(SlicePath(b, part, nsplit, dper, d1 - d0, one_trip, sn, padded, in_lds, compacted, frozenset(classes),
                                 int(c.max()) if c.size else 0, int(pads[d0:d1].sum())))
    return out


def ball_like(rng, B, S, N, ns):
    """Groups shaped like ball-query output, [B][S][ns] int32: per group h in [1, ns] distinct ascending indices, then copies of the first.
    Group (0, 0) of every array has h = 1 and group (0, 1) has h = ns."""
    assert S >= 2 and ns <= N
    idx = np.empty((B, S, ns), dtype=np.int32)
    for b in range(B):
        for i in range(S):
            h = int(rng.integers(1, ns + 1))
            if b == 0 and i < 2:
                h = 1 if i == 0 else ns
            hits = np.sort(rng.choice(N, size=h, replace=False))
            idx[b, i, :h] = hits
            idx[b, i, h:] = hits[0]
    return idx


def with_hub(idx, p=0):
    """ball_like groups in which point p (the lowest index) is the first hit of EVERY group: it collects most of the padding"""
    assert p == 0
    idx = idx.copy()
    idx[idx == idx[:, :, :1]] = p            # slot 0 and its copies; the other hits are larger than the old first hit, hence than 0
    return idx


# ----------------------------------------------------------------------------- the case table
Case = collections.namedtuple("Case", "name B S N k kind skip_pad path")


def _uniform(c, rng):
    return rng.integers(0, c.N, size=(c.B, c.S, c.k)).astype(np.int32)


def _some_trailing_pads(c, idx):
    """every 7th group of a wide case ends in a copy of its slot 0: padding (a trailing run of length >= 1) in every slice, so that the
    compact index has slots to leave out on every path -- chance repeats of slot 0 further up a row are ordinary slots"""
    if c.k >= 12:
        idx[:, ::7, -1] = idx[:, ::7, 0]
    return idx


def _columns_mod64(c, rng, ncol):
    idx = _uniform(c, rng)
    i, s = np.arange(c.S)[:, None], np.arange(ncol)[None, :]
    idx[:, :, :ncol] = (ncol * i + s) % 64
    return idx


def case_idx(name):
    """idx [B][S][k] int32 of one row of the table (fixed seed: the same array in every test that names the case)"""
    c = CASES[name]
    rng = np.random.default_rng(0)
    if c.kind == "uniform":
        return _some_trailing_pads(c, _uniform(c, rng))
    if c.kind == "hubs":                       # D: column 0 -> point 7, columns 1..8 -> point 150
        idx = _uniform(c, rng)
        idx[:, :, 0] = 7
        idx[:, :, 1:9] = 150
        return idx
    if c.kind == "one_point":                  # E
        return np.full((c.B, c.S, c.k), 37, dtype=np.int32)
    if c.kind == "mod64x12":                   # G
        return _some_trailing_pads(c, _columns_mod64(c, rng, 12))
    if c.kind == "mod64x20":                   # H
        return _some_trailing_pads(c, _columns_mod64(c, rng, 20))
    assert c.kind == "ball_like"
    return ball_like(rng, c.B, c.S, c.N, c.k)


# `path`: what the case is there for, as predicates over (case, its SlicePaths, its reference index); each is asserted by
# tests/test_reverse_restatement_cpu.py with the case's own skip_pad, so a changed seed or kernel constant fails there instead of silently
# testing another path here.
def _all(f):
    return lambda c, sl, ref: all(f(s) for s in sl)


def _slice0(f):
    return lambda c, sl, ref: all(f(s) for s in sl if s.part == 0)


def _rest(f):
    return lambda c, sl, ref: all(f(s) for s in sl if s.part != 0)


_LDS1 = _all(lambda s: s.one_trip and s.in_lds and not s.compacted)
_SEVERAL16 = _all(lambda s: s.nsplit == 16 and not s.one_trip)

CASES = collections.OrderedDict((c.name, c) for c in (
    Case("A", 3, 256, 256, 20, "uniform", False, (
        _all(lambda s: s.nsplit == 8 and s.nd == 32), _LDS1, _all(lambda s: s.classes == {LE64}),
        lambda c, sl, ref: len(sl) == 24 and c.B % 8 != 0)),           # 24 workgroups; B no multiple of 8: the plain xcd_cloud_map
    Case("B", 2, 48, 301, 12, "uniform", False, (
        _all(lambda s: s.nsplit == 8 and s.dper == 38 and s.nd == (35 if s.part == 7 else 38)), _LDS1)),
    Case("C1", 1, 3, 5, 2, "uniform", False, (
        _all(lambda s: s.nd == (1 if s.part < 5 else 0)), lambda c, sl, ref: sum(s.nd == 0 for s in sl) == 3, _LDS1)),
    Case("C2", 2, 1, 1, 1, "uniform", False, (
        _all(lambda s: s.nd == (1 if s.part == 0 else 0) and s.sn == (1 if s.part == 0 else 0)), _LDS1)),
    Case("C3", 1, 4, 9, 256, "uniform", False, (
        lambda c, sl, ref: (ref.rev_ent & 255).max() == 255 and (ref.rev_ent >> 8).max() == 3, _LDS1,
        lambda c, sl, ref: sum(s.nd == 0 for s in sl) == 3)),
    Case("D", 2, 128, 200, 32, "hubs", False, (
        _LDS1, lambda c, sl, ref: all(any(MID in s.classes for s in sl if s.b == b) and any(BIG in s.classes for s in sl if s.b == b)
                                      for b in range(c.B)),
        lambda c, sl, ref: all(64 < ref.rev_cnt[b * c.N + 7] <= 512 < ref.rev_cnt[b * c.N + 150] for b in range(c.B)))),
    Case("E", 1, 128, 64, 32, "one_point", False, (
        _LDS1, lambda c, sl, ref: ref.rev_cnt[37] == 4096 and ref.rev_cnt.sum() == 4096,
        lambda c, sl, ref: [s.classes for s in sl if s.sn] == [{BIG}])),
    Case("F", 2, 1024, 1024, 24, "uniform", False, (
        _SEVERAL16, _all(lambda s: s.in_lds and s.compacted and s.dper == 64))),
    Case("G", 2, 1024, 1024, 24, "mod64x12", False, (
        _SEVERAL16, _slice0(lambda s: s.in_lds and not s.compacted and s.sn > RV_CAP // 2 and MID in s.classes),
        _rest(lambda s: s.in_lds and s.compacted))),
    Case("H", 2, 1024, 1024, 24, "mod64x20", False, (
        _SEVERAL16, _slice0(lambda s: not s.in_lds and not s.compacted and s.sn > RV_CAP), _rest(lambda s: s.in_lds and s.compacted))),
    Case("I", 32, 32, 1024, 4, "uniform", False, (
        _all(lambda s: s.nsplit == 8 and s.dper == 128), _LDS1,
        lambda c, sl, ref: c.N >= 1024 and c.B % 8 == 0)),                # (and the interleaved xcd_cloud_map of B % 8 == 0)
    Case("J", 3, 64, 1030, 8, "uniform", False, (
        _all(lambda s: s.nsplit == 16 and s.dper == 65 and s.nd == (55 if s.part == 15 else 65)), _LDS1)),
    Case("A'", 3, 256, 256, 20, "ball_like", True, (
        _LDS1, lambda c, sl, ref: ref.pad_cnt[0] == c.k - 1 and ref.pad_cnt[1] == 0 and 0 < ref.pad_cnt.sum() == (~ref.listed).sum())),
    Case("B'", 2, 48, 301, 12, "ball_like", True, (
        _LDS1, lambda c, sl, ref: ref.pad_cnt[0] == c.k - 1 and ref.pad_cnt[1] == 0 and 0 < ref.pad_cnt.sum() == (~ref.listed).sum())),
    Case("D'", 2, 128, 200, 32, "ball_like", True, (
        _LDS1, lambda c, sl, ref: ref.pad_cnt[0] == c.k - 1 and ref.pad_cnt[1] == 0 and 0 < ref.pad_cnt.sum() == (~ref.listed).sum())),
))
