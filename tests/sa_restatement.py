"""Own-words torch restatement of the set-abstraction kernel family (mlsp_amd/csrc/sa.hip) and the inputs its GPU tests run on.

Plain torch on the CPU, parameterised by dtype: in float64 it is what tests/test_gpu_sa_paths.py measures the kernels against, in fp32 it
is the yardstick (the reference's own rounding) and, for the index results, the exact expectation.  The discrete parts (farthest point
sampling, ball query, the kNN ranking) are oracle/ref_sa_cpu.py's, which tests/golden/sa_*.npz pin to the reference; what is added here:

  group              [x_j - c_i | f_j] edge rows                                         (pointnet_util.py:120-129)
  interp3            inverse-distance interpolation from the three nearest sources, on   (pointnet_util.py:287-294)
                     the direct-form distance sum_c (a_c - b_c)^2, stable sort
  fold_first_layer   relu(BN(W0 [x_j - c_i ; f_j] + b0)) over the E edge rows            (pointnet_util.py:185-190, first layer)
  sa_branch          that layer, the remaining Conv+BN+ReLU layers and the neighbourhood max at FORCED slots

and the case tables.  tests/test_sa_restatement_cpu.py pins the functions to the oracle and the goldens and proves, per case, the
condition the case is there for (pads present, a query without a hit, exact ties, fp32 and float64 rankings identical on the lattice), so
that no GPU test passes vacuously."""
import collections

import torch

from oracle import ref_sa_cpu as sa

U = 2.0 ** -24                  # unit roundoff of fp32
PER_CONTRACTION = 2e-6          # the GEMM family's bar per chained contraction (test_gemm_split_bf16_accuracy)

# which kernel launch_fps runs a cloud of N points on (mlsp_fps_plan): 2 = fps_kernel2 (64 <= N <= 2048), 1 = fps_kernel, 0 = none
FPS_PLAN = collections.OrderedDict([(1, 1), (5, 1), (63, 1), (64, 2), (65, 2), (100, 2), (256, 2), (257, 2), (300, 2), (2047, 2), (2048, 2),
                                    (2049, 1), (8192, 1), (8193, 0)])
FPS_SWEEP_N = (1, 5, 63, 64, 65, 256, 257, 2047, 2048, 2049, 8192)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def lattice(g, shape, span=16):
    """coordinates that are multiples of 1/8 in [-span/8, span/8] (span <= 16: [-2, 2]): differences, squares and their sums are exact
    in fp32 in any order, so fp32 and float64 rank alike, and exact ties abound (the smaller the span, the more)"""
    assert span <= 16
    return torch.randint(-span, span + 1, shape, generator=g).float() / 8


def cloud(g, shape, offset=0.0):
    """uniform in [-1, 1]^C, shifted by `offset` in fp32 (the shifted fp32 values ARE the input, also of a float64 run)"""
    return (torch.rand(shape, generator=g) * 2 - 1) + offset


def dist(a, b):
    """max |a - b| / max |b|"""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def square_distance(a, b):
    """[B,N,C], [B,M,C] -> [B,N,M]: sum_c (a_c - b_c)^2, the difference first (pointnet_util.py:36)"""
    return ((a[:, :, None] - b[:, None]) ** 2).sum(-1)


def gather(points, idx):
    """points [B,N,C], idx [B,...] -> [B,...,C]"""
    B = points.shape[0]
    flat = idx.reshape(B, -1)
    return torch.gather(points, 1, flat[..., None].expand(-1, -1, points.shape[-1])).reshape(*idx.shape, points.shape[-1])


# ----------------------------------------------------------------------------- the float-valued functions
def group(xyz, new_xyz, feat, idx):
    """xyz [B,N,3], new_xyz [B,S,3], feat [B,N,D] | None, idx [B,S,ns] -> [B*S*ns, 3+D] rows [xyz_j - new_xyz_i | feat_j]"""
    B, S, ns = idx.shape
    g = gather(xyz, idx) - new_xyz[:, :, None]
    if feat is not None and feat.shape[-1] > 0:
        g = torch.cat([g, gather(feat, idx)], -1)
    return g.reshape(B * S * ns, -1)


def group_backward(xyz, new_xyz, feat, idx, W, dtype):
    """gradients of sum(W * group(...)) in `dtype` -> {"dxyz", "dnew_xyz", "dfeat"} (autograd of the restatement)"""
    x, q = leaf(xyz, dtype), leaf(new_xyz, dtype)
    f = leaf(feat, dtype) if feat is not None and feat.shape[-1] > 0 else None
    (group(x, q, f, idx) * W.to(dtype)).sum().backward()
    out = {"dxyz": x.grad, "dnew_xyz": q.grad}
    if f is not None:
        out["dfeat"] = f.grad
    return out


def group_backward_bounds(idx, W, N):
    """Per element of the three gradients, the summation bound (n + 1) * 2^-24 * sum |terms|: every element is a plain sum of n entries of
    W (fp32 data, exact in float64) -- over the list of edges that name the point for dxyz / dfeat, over the ns slots of the centre for
    dnew_xyz -- and ANY order of n fp32 additions errs by at most (n - 1) u sum|terms| to first order; n + 1 covers the higher orders.
    An element nobody names has n = 0 and no terms: its bound is 0, it must be exactly 0."""
    B, S, ns = idx.shape
    Wa = W.double().abs().view(B, S * ns, -1)
    flat = idx.reshape(B, S * ns)
    tot = torch.zeros(B, N, Wa.shape[-1], dtype=torch.float64)
    tot.scatter_add_(1, flat[..., None].expand(-1, -1, Wa.shape[-1]), Wa)
    n = torch.zeros(B, N, dtype=torch.float64).scatter_add_(1, flat, torch.ones(B, S * ns, dtype=torch.float64))
    per_point = (n[..., None] + 1) * U * tot
    return {"dxyz": per_point[..., :3], "dfeat": per_point[..., 3:],
            "dnew_xyz": (ns + 1) * U * Wa.view(B, S, ns, -1)[..., :3].sum(2)}, n


def interp3(feat, xyz1, xyz2):
    """feat [B,S,D] on the sources xyz2 [B,S,3] -> [B,N,D] on the points xyz1 [B,N,3]: the three nearest sources by direct-form distance
    (stable sort: ties -> lower index), weights (1 / (d + 1e-8)) normalised.  S == 1: the one row, repeated.  -> out, idx [B,N,3], d"""
    B, N, _ = xyz1.shape
    S = xyz2.shape[1]
    if S == 1:
        return feat.repeat(1, N, 1), None, None
    d, order = torch.sort(square_distance(xyz1, xyz2), dim=-1, stable=True)
    d, idx = d[:, :, :3], order[:, :, :3]
    recip = 1.0 / (d + 1e-8)
    w = recip / recip.sum(-1, keepdim=True)
    return (gather(feat, idx) * w[..., None]).sum(2), idx, d


def _bn_relu(y, gamma, beta, run_mean, run_var, training, momentum, eps, pre_out=None):
    """BatchNorm over the rows of y [E, C] + ReLU -> z, new running mean, new running var (nn.BatchNorm's update rule).
    pre_out (a list) receives the ReLU's argument: where it is within rounding of 0 the derivative is decided by rounding."""
    E = y.shape[0]
    if training:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        new_mean = (1 - momentum) * run_mean + momentum * mean.detach()
        new_var = (1 - momentum) * run_var + momentum * var.detach() * (E / (E - 1))
    else:
        mean, var, new_mean, new_var = run_mean, run_var, run_mean, run_var
    pre = (y - mean) / torch.sqrt(var + eps) * gamma + beta
    if pre_out is not None:
        pre_out.append(pre.detach())
    return torch.relu(pre), new_mean, new_var


def fold_first_layer(xyz, new_xyz, feat, idx, W0, b0, gamma, beta, run_mean, run_var, training, momentum=0.1, eps=1e-5, pre_out=None):
    """relu(BN(W0 [x_j - c_i ; f_j] + b0)) over the E = B*S*ns edge rows; W0 [C, 3+D] with columns [xyz | feat].
    -> Z [E, C], new running mean, new running var.  Gradients to xyz, new_xyz, feat, W0, gamma, beta by autograd."""
    y = group(xyz, new_xyz, feat, idx) @ W0.t() + b0
    return _bn_relu(y, gamma, beta, run_mean, run_var, training, momentum, eps, pre_out)


def sa_branch(xyz, new_xyz, feat, idx, layers, training, sel=None, momentum=0.1, eps=1e-5, pre_out=None):
    """One branch of a set-abstraction layer on given centres and neighbourhoods: the folded first layer, the remaining Conv(1x1) + BN + ReLU
    layers on the edge rows, the max over the ns slots.  layers: list of {"W" [Cout, Cin] (first: columns [xyz | feat]), "b", "gamma",
    "beta", "run_mean", "run_var"}.  sel [B*S, C] (slots) FORCES the max to those slots (a gather: two precisions route alike).
    -> out [B, S, C], the slots used [B*S, C], [(new running mean, new running var)] per layer"""
    B, S, ns = idx.shape
    L = layers[0]
    z, m, v = fold_first_layer(xyz, new_xyz, feat, idx, L["W"], L["b"], L["gamma"], L["beta"], L["run_mean"], L["run_var"], training,
                               momentum, eps, pre_out)
    bufs = [(m, v)]
    for L in layers[1:]:
        z, m, v = _bn_relu(z @ L["W"].t() + L["b"], L["gamma"], L["beta"], L["run_mean"], L["run_var"], training, momentum, eps, pre_out)
        bufs.append((m, v))
    z = z.view(B * S, ns, -1)
    if sel is None:
        sel = z.argmax(1)
    return torch.gather(z, 1, sel[:, None, :]).squeeze(1).view(B, S, -1), sel, bufs


def trailing_pads(idx):
    """[B,S,ns] bool: the padding slots of every group -- its trailing run of slots s > 0 equal to slot 0"""
    differs = idx[:, :, 1:] != idx[:, :, :1]
    keep = torch.flip(torch.cummax(torch.flip(differs, [-1]).int(), -1)[0], [-1]).bool()
    return torch.cat([torch.zeros_like(idx[:, :, :1], dtype=torch.bool), ~keep], -1)


def pads_to_slot0(sel, idx):
    """arg-max slots [B*S, C] with every padding slot replaced by slot 0 (the same point, the same row: an exact tie that the HIP path
    gives to slot 0 -- its compact reverse lists leave the padding slots out)"""
    pad = trailing_pads(idx).reshape(-1, idx.shape[-1])
    return torch.where(torch.gather(pad, 1, sel), torch.zeros_like(sel), sel)


# ----------------------------------------------------------------------------- FPS cases
FpsCase = collections.namedtuple("FpsCase", "name N S kind")


def _fps_cases():
    out = []
    for N in FPS_SWEEP_N:
        S = N if N <= 257 else 64
        for kind in ("random", "lattice"):
            out.append(FpsCase("%s-N%d-S%d" % (kind, N, S), N, S, kind))
    out += [FpsCase("random-N%d-S1" % N, N, 1, "random") for N in (64, 2049)]
    out += [FpsCase("identical-N300-S8", 300, 8, "identical"), FpsCase("pitch6-N100-S10", 100, 10, "pitch6"),
            FpsCase("noncontiguous-N100-S10", 100, 10, "noncontiguous"), FpsCase("lattice4-N2048-S64", 2048, 64, "lattice4")]
    return collections.OrderedDict((c.name, c) for c in out)


FPS_CASES = _fps_cases()
FPS_B = 3


def fps_input(c):
    """-> xyz [3, N, 3] (for pitch6 / noncontiguous: a view with that layout), start [3] (0, the middle, N - 1)"""
    g = gen(1000 + c.N + c.S)
    N = c.N
    start = torch.tensor([0, N // 2, N - 1])
    if c.kind == "lattice":
        xyz = lattice(g, (FPS_B, N, 3))
    elif c.kind == "lattice4":                      # 729 sites for 2048 points: every running minimum is tied many times over
        xyz = lattice(g, (FPS_B, N, 3), span=4)
    elif c.kind == "identical":
        xyz = lattice(g, (FPS_B, 1, 3)).expand(-1, N, -1).contiguous()
    elif c.kind == "pitch6":
        xyz = cloud(g, (FPS_B, N, 6))[..., :3]
    elif c.kind == "noncontiguous":
        xyz = cloud(g, (N, FPS_B, 3)).transpose(0, 1)
    else:
        xyz = cloud(g, (FPS_B, N, 3))
    return xyz, start


# ----------------------------------------------------------------------------- ball-query cases
BallCase = collections.namedtuple("BallCase", "name N S nsample radius kind")
FAR = 2.0                                            # the corner (2, 2, 2): a lattice point no query of a built case reaches

BALL_CASES = collections.OrderedDict((c.name, c) for c in (
    BallCase("many-in-first-chunk", 130, 9, 8, 1.0, "lattice4"),
    BallCase("nsample-th-hit-is-lane-63", 130, 2, 8, 0.5, "last_lane"),
    BallCase("first-hit-beyond-128", 300, 3, 8, 1.0, "beyond128"),
    BallCase("one-hit", 65, 4, 8, 0.05, "one_hit"),
    BallCase("nsample-64-gt-N-63", 63, 5, 64, 1.0, "lattice"),
    BallCase("nsample-65-gt-N-63", 63, 5, 65, 0.5, "lattice"),
    BallCase("nsample-255-gt-N-63", 63, 5, 255, 1.0, "lattice"),
    BallCase("nsample-8-gt-N-1", 1, 1, 8, 1.0, "self"),
    BallCase("on-the-sphere-r0.5", 300, 20, 64, 0.5, "lattice"),
    BallCase("r0.1", 300, 20, 8, 0.1, "random"),
    BallCase("r0.2", 300, 20, 64, 0.2, "random"),
    BallCase("pitch6-xyz", 130, 9, 8, 0.5, "pitch6_xyz"),
    BallCase("pitch6-new_xyz", 130, 9, 8, 0.5, "pitch6_new"),
    BallCase("zero-hit", 64, 3, 8, 0.5, "zero_hit"),
))
BALL_SWEEP_N = (1, 63, 64, 65, 130, 300)
BALL_SWEEP_NS = (1, 8, 64, 65, 255)
BALL_B = 2


def ball_sweep_case(N, ns):
    """the grid of the issue: lattice clouds, queries = the cloud's first min(N, 7) points, radius 0.5 / 1.0 alternating"""
    return BallCase("sweep-N%d-ns%d" % (N, ns), N, min(N, 7), ns, 0.5 if (N + ns) % 2 else 1.0, "self")


def ball_input(c):
    """-> xyz [2, N, 3], new_xyz [2, S, 3] (pitch6_*: views of pitch 6)"""
    g = gen(2000 + c.N + 7 * c.nsample)
    B, N, S = BALL_B, c.N, c.S
    if c.kind == "random":
        xyz = cloud(g, (B, N, 3))
        return xyz, xyz[:, :S].clone()
    if c.kind == "self":
        xyz = lattice(g, (B, N, 3))
        return xyz, xyz[:, :S].clone()
    if c.kind in ("lattice", "lattice4", "pitch6_xyz", "pitch6_new"):
        # a dense lattice cloud (9^3 sites); every query is one step of at most 1/8 per axis away from a point of the cloud: >= 1 hit
        xyz = lattice(g, (B, N, 6), span=4)[..., :3]
        new_xyz = torch.cat([xyz[:, :S] + lattice(g, (B, S, 3), span=1), lattice(g, (B, S, 3))], -1)[..., :3]
        return (xyz if c.kind == "pitch6_xyz" else xyz.contiguous()), (new_xyz if c.kind == "pitch6_new" else new_xyz.contiguous())
    xyz = torch.full((B, N, 3), FAR)
    if c.kind == "last_lane":
        # query 0 at the origin: hits 3, 10, ..., 60, 63 (the 8th is lane 63 of the first chunk), then 70 and 100;
        # query 1 at (-1, -1, -1): hits 65 .. 72 without 70, then 127 (the 8th: lane 63 of the second chunk), 128, 129
        near = lattice(g, (B, 20, 3), span=2)                          # within sqrt(3) / 4 < 0.5 of its centre
        h0, h1 = [3, 10, 20, 30, 40, 50, 60, 63, 70, 100], [65, 66, 67, 68, 69, 71, 72, 127, 128, 129]
        xyz[:, h0] = near[:, :10]
        xyz[:, h1] = near[:, 10:] - 1.0
        return xyz, torch.tensor([[0.0, 0.0, 0.0], [-1.0, -1.0, -1.0]]).expand(B, -1, -1).contiguous()
    if c.kind == "beyond128":
        xyz[:, 129:] = lattice(g, (B, N - 129, 3), span=4)
        return xyz, lattice(g, (B, S, 3), span=2)
    if c.kind == "one_hit":
        # all points distinct (a permutation of lattice sites along x); the queries are points of the cloud, nothing else within 0.05
        xyz = torch.zeros(B, N, 3)
        site = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
        xyz[:, :, 0] = (site % 33 - 16).float() / 8
        xyz[:, :, 1] = (site // 33).float() / 8
        return xyz, xyz[:, [0, 17, 40, 64]].clone()
    assert c.kind == "zero_hit"
    xyz = lattice(g, (B, N, 3))
    new_xyz = xyz[:, :S].clone()
    new_xyz[:, 1] = 10.0                                               # no point within 0.5 of (10, 10, 10)
    return xyz, new_xyz


def ball_hits(c, xyz, new_xyz, dtype=torch.float32):
    """[B,S,N] bool: !(d > r^2) in `dtype`"""
    return ~(square_distance(new_xyz.to(dtype), xyz.to(dtype)) > c.radius ** 2)


# ----------------------------------------------------------------------------- query-kNN cases
KNN_K = (1, 3, 4, 5, 16, 17, 32, 33, 64)             # both edges of the four KMAX instantiations (4, 16, 32, 64)
KNN_NQ = (1, 255, 257)
KNN_B = 2


def knn_nr(k):
    return sorted({k, 255, 256, 257, 600} - {n for n in (255, 256, 257, 600) if n < k})


def knn_lattice_input(k, Nr, Nq, C=3):
    """references on a coarse lattice (span 4: 9^C sites, so duplicates and exact ties abound); the first min(Nq, Nr) queries are
    references (drawn without replacement), the rest lattice points"""
    g = gen(3000 + 97 * k + 7 * Nr + Nq + C)
    ref = lattice(g, (KNN_B, Nr, C), span=4)
    n_own = min(Nq, Nr)
    own = torch.stack([torch.randperm(Nr, generator=g)[:n_own] for _ in range(KNN_B)])
    q = torch.cat([gather(ref, own), lattice(g, (KNN_B, Nq - n_own, C), span=4)], 1)
    return ref, q, n_own


def knn_oracle(k, ref, q):
    """idx [B,Nq,k], dist [B,Nq,k] of the direct-form distance in ref's dtype, stable sort (ties -> lower index)"""
    d, order = torch.sort(square_distance(q, ref), dim=-1, stable=True)
    return order[:, :, :k], d[:, :, :k]


# ----------------------------------------------------------------------------- grouping cases (forced idx)
GROUP_D = (0, 1, 5, 64, 67, 130)
GROUP_DIMS = (2, 40, 24, 6)                          # B, N, S, ns


def group_idx():
    """[2, 40, (24, 6)] forced neighbourhoods: point 0 named 70 times (one list longer than 64), points 1..4 named 4, 5, 6, 7 times
    (list lengths 0, 1, 2, 3 mod 4), points 30..39 named by nobody, repeats inside a row"""
    B, N, S, ns = GROUP_DIMS
    g = gen(4000)
    flat = []
    for b in range(B):
        fixed = [0] * 70 + [1] * 4 + [2] * 5 + [3] * 6 + [4] * 7
        rest = torch.randint(5, 30, (S * ns - len(fixed),), generator=g).tolist()
        row = torch.tensor(fixed + rest)
        row = row[torch.randperm(S * ns, generator=g)] if b else row      # cloud 0: [0, 0, 0, 0, 0, 0] rows first (repeats inside a row)
        flat.append(row)
    return torch.stack(flat).view(B, S, ns)


# ----------------------------------------------------------------------------- interpolation cases
INTERP_D = (1, 3, 4, 7, 64, 130)
INTERP_S = (3, 4, 64)
INTERP_OFFSETS = (0.0, 5.0, 20.0)
INTERP_DIMS = (2, 200)                               # B, N


def interp_input(S, offset):
    """xyz1 [2, 200, 3] (a random cloud shifted by `offset`), xyz2 [2, S, 3] = points of xyz1 (exact coincidences) with source 1 a copy of
    source 0 (two identical sources: weights 1/2 and 1/2 at their own point) and, for S = 64, sources 60..63 moved far away (nobody's
    neighbour: their dfeat rows are exactly zero)"""
    B, N = INTERP_DIMS
    g = gen(5000 + S + int(offset))
    xyz1 = cloud(g, (B, N, 3), offset)
    pick = torch.stack([torch.randperm(N, generator=g)[:S] for _ in range(B)])
    xyz2 = gather(xyz1, pick).clone()
    xyz2[:, 1] = xyz2[:, 0]
    if S == 64:
        xyz2[:, 60:] = xyz2[:, 60:] + 50.0
    return xyz1, xyz2


# ----------------------------------------------------------------------------- folded-first-layer cases
FoldCase = collections.namedtuple("FoldCase", "name C ns D training kind B N S seed", defaults=(0,))
FOLD_NS = (1, 3, 16, 33, 64)             # with B = 2 clouds of S = 25 centres: E = 50, 150 (below 256), 800, 1650, 3200 (no multiple of 256)
# Conditioning.  The folded layer forms y = u_j - w_i from two contractions whose results are relative to max |u|, and BatchNorm divides by
# the channel's standard deviation: an error e * max |u| in y arrives as e * kappa, kappa = max |u| / sqrt(var + eps), in the normalised
# value.  u and w are each rounded to fp32 before they are subtracted, so e >= 2 * 2^-24 = 1.2e-7 whatever the products do; for that
# alone to stay below half of the 2e-6 floor per contraction, a case needs kappa <= 1e-6 / 1.2e-7 ~ 8 per chained contraction
# (FOLD_KAPPA_MAX; tests/test_sa_restatement_cpu.py asserts it).  That rules out inputs on which no fp32 evaluation of the folded form can
# meet the floor: ball-query groups without features whose radius is small against the cloud (almost every row of the batch is the zero
# vector -- a handful of distinct rows, channel variances around eps: kappa 95 .. 145 at radius 0.25 with 200 points, where the HIP path
# measured 1.6e-5 .. 1.8e-4 from float64), and the k = 1 "neighbourhood" of a centre without features (every row zero, variance 0).
# Hence: the ball-query cases draw FOLD_BALL_N points in [-1, 1]^3 and use FOLD_RADIUS (about eight points inside: groups of
# ns >= 16 are mostly padding), with seeds whose draw meets the condition.
FOLD_KAPPA_MAX = 8.0
FOLD_BALL_N = 30
FOLD_SEEDS = {"C16-ball-ns1-D0-train": 11, "C64-ball-ns3-D0-train": 8, "C256-ball-ns16-D0-train": 5}


def _fold_cases():
    out, n = [], 0
    for C in (16, 32, 64, 128, 256):
        for kind in ("ball", "knn", "pinned"):
            ns = FOLD_NS[n % 5]
            if kind == "pinned" and ns < 3:
                ns = 3 if ns == 1 else ns
            D = 5 if n % 2 or (kind == "knn" and ns == 1) else 0       # (the one nearest neighbour of a centre is itself: x_j - c_i = 0)
            training = n % 4 != 3
            N = FOLD_BALL_N if kind == "ball" else 200
            name = "C%d-%s-ns%d-D%d-%s" % (C, kind, ns, D, "train" if training else "eval")
            out.append(FoldCase(name, C, ns, D, training, kind, 2, N, 25, FOLD_SEEDS.get(name, 0)))
            n += 1
    return collections.OrderedDict((c.name, c) for c in out)


FOLD_CASES = _fold_cases()
# the module-level cases (PointNetSetAbstraction / ...Msg with fold_first): one of every neighbourhood kind
# (small: the loss of a whole module reaches every ReLU of every layer, and a ReLU whose argument lies within rounding of 0 has its
# derivative decided by rounding; tests/test_sa_restatement_cpu.py proves that no argument of these cases comes closer than KINK_MARGIN)
MODULE_CASES = collections.OrderedDict((c.name, c) for c in (
    FoldCase("sa-ball", 32, 8, 5, True, "ball", 2, FOLD_BALL_N, 7, 49), FoldCase("sa-knn", 64, 4, 0, True, "knn", 2, 200, 7, 37),
    FoldCase("sa-pinned", 16, 6, 5, True, "pinned", 2, 200, 7, 5), FoldCase("sa-pinned-eval", 32, 4, 0, False, "pinned", 2, 200, 7, 15),
    FoldCase("msg-ball", 16, 8, 5, True, "ball", 2, FOLD_BALL_N, 7, 4), FoldCase("msg-knn", 32, 4, 0, True, "knn", 2, 200, 7, 25)))
MODULE_WIDTH2 = 16             # the second (last) layer of a module case
KINK_MARGIN = 1e-4             # |ReLU argument| / max |ReLU argument| of every layer of a module case stays above this
FOLD_RADIUS = 0.8              # ~8 of FOLD_BALL_N uniform points fall within 0.8 of a centre: groups of ns >= 16 are mostly padding


def fold_input(c):
    """-> xyz [B,N,3], feat [B,N,D] | None, fps_idx [B,S], idx [B,S,ns] (int64).  ball: ball-query groups at FOLD_RADIUS (trailing pads);
    knn: the ns nearest (no pads); pinned: a caller's own rows -- every second row repeats its slot 0 in slot 1 and ends in another point
    (`[5, 5, 7, 9]`: a repeat that is NOT padding), the rows between end in a run of copies of slot 0 (padding) after a repeat mid-row"""
    g = gen(6000 + c.C + 3 * c.ns + c.D + c.S + 1000 * c.seed)
    xyz = cloud(g, (c.B, c.N, 3))
    feat = torch.randn(c.B, c.N, c.D, generator=g) if c.D else None
    fps_idx = sa.fps(xyz, c.S, torch.arange(c.B) % c.N)
    new_xyz = sa.gather_rows(xyz, fps_idx)
    if c.kind == "ball":
        idx = sa.ball_query(FOLD_RADIUS, c.ns, xyz, new_xyz)
    elif c.kind == "knn":
        idx = sa.knn_group(c.ns, xyz, new_xyz)
    else:
        assert c.ns >= 3
        idx = torch.randint(0, c.N, (c.B, c.S, c.ns), generator=g)
        idx[:, :, 1] = idx[:, :, 0]                                     # the repeat of slot 0 in the middle of the row
        last = (idx[:, :, 0] + 1 + torch.randint(0, c.N - 1, (c.B, c.S), generator=g)) % c.N        # != slot 0
        idx[:, 0::2, -1] = last[:, 0::2]
        idx[:, 1::2, -1] = idx[:, 1::2, 0]                              # a trailing pad ...
        if c.ns >= 4:
            idx[:, 1::2, -2] = last[:, 1::2]                            # ... of length exactly 1: slot ns - 2 is another point
        idx[0, 0, :min(c.ns, 4)] = torch.tensor([5, 5, 7, 9][:min(c.ns, 4)] if c.ns >= 4 else [5, 5, 7])
    return xyz, feat, fps_idx, idx


def fold_layers(c, widths, msg=False):
    """parameters of a branch [3 + D -> widths...] (float32): weights, conv biases, BatchNorm scales of both signs, off-default buffers"""
    g = gen(7000 + c.C + c.ns + 1000 * c.seed)
    layers, cin = [], 3 + c.D
    for w in widths:
        gamma = (0.5 + torch.rand(w, generator=g)) * torch.where(torch.rand(w, generator=g) < 0.3, -1.0, 1.0)
        gamma[0], gamma[1] = -abs(gamma[0]), abs(gamma[1])
        layers.append({"W": torch.randn(w, cin, generator=g) / cin ** 0.5, "b": 0.1 * torch.randn(w, generator=g), "gamma": gamma,
                       "beta": 0.3 * torch.randn(w, generator=g), "run_mean": 0.2 * torch.randn(w, generator=g),
                       "run_var": 0.5 + torch.rand(w, generator=g)})
        cin = w
    return layers


def leaf(t, dtype, grad=True):
    """a fresh leaf holding t's values in `dtype` (never t itself: .to() of the same dtype returns its argument)"""
    return t.detach().clone().to(dtype).requires_grad_(grad)


def _layer_leaves(layers, dtype):
    return [{k: leaf(v, dtype, k in ("W", "b", "gamma", "beta")) for k, v in L.items()} for L in layers]


def _layer_quantities(q, Ls, bufs, training):
    for i, (L, (m, v)) in enumerate(zip(Ls, bufs)):
        q["dW%d" % i], q["dgamma%d" % i], q["dbeta%d" % i] = L["W"].grad, L["gamma"].grad, L["beta"].grad
        if training:
            q["run_mean%d" % i], q["run_var%d" % i] = m.detach(), v.detach()
        else:
            q["db%d" % i] = L["b"].grad          # (in front of batch statistics a conv bias has an analytically zero gradient: not compared)
    return q


def fold_weights(c):
    """Loss weights [E, C] (fp32) of a layer-level case, loss = sum(weights * Z).  Random, except: (1) the padding rows of a group carry
    the weights of the group's LAST row -- the premise of the compact reverse lists (identical rows in, identical gradients back, as behind
    the layer's own neighbourhood max, which never selects a padding slot) -- and (2) zero where the ReLU's argument, in float64, lies
    within KINK_MARGIN of 0 relative to the layer's largest: there the derivative is decided by rounding, in any precision."""
    xyz, feat, fps_idx, idx = fold_input(c)
    L = {k: v.double() for k, v in fold_layers(c, [c.C])[0].items()}
    pre = []
    fold_first_layer(xyz.double(), gather(xyz, fps_idx).double(), None if feat is None else feat.double(), idx, L["W"], L["b"], L["gamma"],
                     L["beta"], L["run_mean"], L["run_var"], c.training, pre_out=pre)
    E = c.B * c.S * c.ns
    w = torch.randn(E, c.C, generator=gen(8000 + c.C + c.ns)).view(c.B * c.S, c.ns, c.C)
    w = torch.where(trailing_pads(idx).view(c.B * c.S, c.ns, 1), w[:, -1:, :], w).reshape(E, c.C)
    near = pre[0].abs() < KINK_MARGIN * pre[0].abs().max()
    return torch.where(near, torch.zeros(()), w).contiguous(), int(near.sum())


def fold_quantities(c, dtype, wgt):
    """the folded first layer of a layer-level case in `dtype`, the centres a leaf of their own -> {name: tensor}"""
    xyz, feat, fps_idx, idx = fold_input(c)
    x, q_ = leaf(xyz, dtype), leaf(gather(xyz, fps_idx), dtype)
    f = leaf(feat, dtype) if feat is not None else None
    Ls = _layer_leaves(fold_layers(c, [c.C]), dtype)
    L = Ls[0]
    z, m, v = fold_first_layer(x, q_, f, idx, L["W"], L["b"], L["gamma"], L["beta"], L["run_mean"], L["run_var"], c.training)
    (z * wgt.to(dtype)).sum().backward()
    q = {"Z": z.detach(), "dxyz": x.grad, "dnew_xyz": q_.grad}
    if f is not None:
        q["dfeat"] = f.grad
    return _layer_quantities(q, Ls, [(m, v)], c.training)


def module_weights(c):
    return torch.randn(c.B, c.S, MODULE_WIDTH2, generator=gen(8100 + c.C))


def module_quantities(c, dtype, sel=None, pre_out=None):
    """a module case (first width c.C, second MODULE_WIDTH2; centres = rows of xyz, so d xyz includes their share) in `dtype` with the
    neighbourhood max at the slots `sel` (None: its own arg-max) -> ({name: tensor}, the slots used)"""
    xyz, feat, fps_idx, idx = fold_input(c)
    x = leaf(xyz, dtype)
    f = leaf(feat, dtype) if feat is not None else None
    Ls = _layer_leaves(fold_layers(c, [c.C, MODULE_WIDTH2]), dtype)
    out, sel, bufs = sa_branch(x, gather(x, fps_idx), f, idx, Ls, c.training, sel=sel, pre_out=pre_out)
    (out * module_weights(c).to(dtype)).sum().backward()
    q = {"out": out.detach(), "dxyz": x.grad}
    if f is not None:
        q["dfeat"] = f.grad
    return _layer_quantities(q, Ls, bufs, c.training), sel


def fold_kappa(c, widths):
    """max over the channels of max |u| / sqrt(var + eps) for the first layer of a case (float64; see FOLD_KAPPA_MAX)"""
    xyz, feat, fps_idx, idx = fold_input(c)
    L = {k: v.double() for k, v in fold_layers(c, widths)[0].items()}
    u = xyz.double().reshape(-1, 3) @ L["W"][:, :3].t() + L["b"]
    if feat is not None:
        u = u + feat.double().reshape(-1, c.D) @ L["W"][:, 3:].t()
    y = group(xyz.double(), gather(xyz, fps_idx).double(), None if feat is None else feat.double(), idx) @ L["W"].t() + L["b"]
    var = ((y - y.mean(0)) ** 2).mean(0) if c.training else L["run_var"]
    return float((u.abs().max(0)[0] / torch.sqrt(var + 1e-5)).max())
