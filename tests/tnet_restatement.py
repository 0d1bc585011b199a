"""The fused T-Net per-edge stage (mlsp_amd/csrc/tnet.hip, Fh.tnet_edge) restated with plain torch ops over the reference's op sequence
(oracle/ref_torch_modules.py: edge features, then 1x1 Conv2d + BatchNorm2d + LeakyReLU twice, max over k), in float64 -- or in fp32, the
yardstick of tests/test_gpu_tnet.py -- plus the dyadic case builder and the case table of that file.
Shared by tests/test_gpu_kernels.py, tests/test_gpu_tnet.py and tests/test_tnet_restatement_cpu.py."""
import collections

import numpy as np
import torch
import torch.nn.functional as F

from oracle import knn_canon, ref_torch_modules

GRADS = ("dx", "dW1", "dg1", "db1", "dW2", "dg2", "db2")
STATS = ("rm1", "rv1", "rm2", "rv2")
KINK1 = 2.0 ** -13          # no first-layer pre-activation closer to zero than this, in units of the BN1 scale (dyadic_case)
KINK2 = 1e-5                # no second-layer pre-activation at a float64 arg-extreme closer to zero than this (seeds chosen so)


def tnet_edge_f64(xp, idx, W1, g1, b1, W2, g2, b2, slope, sel=None, stats=None, eps=1e-5, parts=False, xc=None):
    """The T-Net per-edge stage through the reference's op sequence (oracle/ref_torch_modules.py: edge features, then 1x1 Conv2d +
    BatchNorm2d + LeakyReLU twice, max over k), in the precision of its arguments: xp [P, C], idx [B, N, k] -> [P, 128].
    sel [P, 128] (optional): the slot each max takes, instead of the arg-max of its own values.
    stats (optional): (rm1, rv1, rm2, rv2), the running statistics both BatchNorms normalise with (eval mode) instead of the batch's.
    xc [P, C] (optional): the centre points as a tensor of their own -- xp then only feeds the neighbour rows, so autograd splits the
    input gradient into its neighbour (u_j) and centre (v_i) shares.
    parts: -> (out, dict(y, a1, z, a2)): both convolutions' outputs (pre-BN) and both pre-activations, [B, C, N, k]."""
    B, N, k = idx.shape
    if xc is None:
        h = ref_torch_modules.edge_features(xp.view(B, N, -1).transpose(2, 1), k, lambda *_: idx)
    else:
        flat = (idx + torch.arange(B).view(B, 1, 1) * N).view(-1)
        ctr = xc.view(B, N, 1, -1).expand(B, N, k, xc.shape[1])
        h = torch.cat((xp[flat].view(B, N, k, -1) - ctr, ctr), dim=3).permute(0, 3, 1, 2)
    pre = []
    for i, (W, g, b) in enumerate(((W1, g1, b1), (W2, g2, b2))):
        y = F.conv2d(h, W[:, :, None, None])
        if stats is None:
            a = F.batch_norm(y, None, None, g, b, True, 0.1, eps)
        else:
            a = F.batch_norm(y, stats[2 * i], stats[2 * i + 1], g, b, False, 0.1, eps)
        h = F.leaky_relu(a, slope)
        pre += [y, a]
    z = h.max(dim=-1)[0] if sel is None else h.gather(-1, sel.long().view(B, N, -1).transpose(2, 1)[..., None])[..., 0]
    out = z.transpose(2, 1).reshape(B * N, -1)
    return (out, dict(y=pre[0], a1=pre[1], z=pre[2], a2=pre[3])) if parts else out


def rel_l2(a, b):
    """|a - b| / |b| in float64: the project's distance for a forward value"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def dist(a, b):
    """max|a - b| / max|b| in float64: the project's distance for a gradient"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


# ----------------------------------------------------------------------------- which kernel a call reaches (launch_tnet_edge_fwd / _bwd)
def points_per_tile(k, forward=False):
    """points of one workgroup tile: 160 / k in the register-resident forward kernels (k = 20, 40), min(8, 128 / k) everywhere else"""
    return 160 // k if forward and k in (20, 40) else min(8, 128 // k)


def fwd_kernel(k, mode):
    if k in (20, 40):
        return "fwd2<%d>" % k if mode == "fp32" else "fwd3<%d,ONEP>" % k if mode == "bf16" else "fwd3<%d>" % k
    return "fwd"


def bwd_kernel(k, mode, slope):
    if slope <= 0:
        return "bwd"
    if mode != "fp32" and k % 2 == 0 and 8 <= k <= 64:
        return "bwds<ONEP>" if mode == "bf16" else "bwds"
    return "bwdg<0,20>" if k <= 20 else "bwdg<0,24>" if k <= 24 else "bwdg<0,32>" if k <= 32 else "bwdg<1,40>" if k <= 40 else "bwdg<2,32>"


def tiles(B, N, k, forward=False):
    """tiles of a launch: tiles never straddle clouds"""
    return B * -(-N // points_per_tile(k, forward))


def grid(ntiles, gram=False):
    """workgroups of a launch: a multiple of 8 up to the cap -- 512 for the forward and round-1 kernels, 256 for the Gram forms"""
    cap = 256 if gram else 512
    return -(-ntiles // 8) * 8 if ntiles < cap else cap


def resolve_mode(mode):
    """"default" -> the process default product mode"""
    if mode != "default":
        return mode
    from mlsp_amd import _lib
    return _lib.DEFAULT_GEMM_PRECISION


# ----------------------------------------------------------------------------- inputs
Inputs = collections.namedtuple("Inputs", "B N k slope training xp idx W1 g1 b1 W2 g2 b2 rs w deg0")


def forced_indices(B, N, k, g):
    """Indices no kNN graph would give: every entry from the first half of its cloud (the second half is nobody's neighbour: degree 0 in
    the reverse index), slot 0 of EVERY row names one hub point, and slot 2 repeats slot 1."""
    idx = torch.randint(0, N // 2, (B, N, k), generator=g)
    idx[:, :, 0] = 1
    if k > 2:
        idx[:, :, 2] = idx[:, :, 1]
    return idx


def dyadic_case(B, N, k, seed, slope=0.2, training=True, graph="knn", neg=False):
    """Coordinates in i / 256 and first weights in j / 16: the first conv's outputs are multiples of 2^-12, exact in fp32 and float64, and
    beta1 puts BN1's zero half-way between two of them -- no first-layer pre-activation lies within KINK1 of the kink (in units of the
    BN scale: the batch's, or the given running statistics' in eval mode), far beyond fp32 rounding, so the LeakyReLU derivative of every
    edge is the same in every evaluation.  neg: a quarter of the gamma1 and gamma2 channels are negative (never zero).
    graph: "knn" (the true kNN graph of the cloud) or "forced" (forced_indices).  -> Inputs (fp32 tensors on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    P = B * N
    xp = torch.randint(-256, 257, (P, 3), generator=g).float() / 256
    W1 = torch.randint(-16, 17, (64, 6), generator=g).float() / 16
    W2 = torch.randn(128, 64, generator=g) / 8
    g1, g2 = torch.rand(64, generator=g) + 0.5, torch.rand(128, generator=g) + 0.5
    b2 = torch.randn(128, generator=g)
    w = torch.randn(P, 128, generator=g)
    rs = [torch.randn(64, generator=g) * 0.1, torch.rand(64, generator=g) + 0.5, torch.randn(128, generator=g) * 0.1,
          torch.rand(128, generator=g) + 0.5]
    if neg:
        g1[torch.randperm(64, generator=g)[:16]] *= -1
        g2[torch.randperm(128, generator=g)[:32]] *= -1
    if graph == "knn":
        idx = torch.from_numpy(knn_canon.knn_point_major(xp.view(B, N, 3), k).astype(np.int64))
    else:
        idx = forced_indices(B, N, k, g)
    y = F.conv2d(ref_torch_modules.edge_features(xp.double().view(B, N, 3).transpose(2, 1), k, lambda *_: idx), W1.double()[:, :, None, None])
    if training:
        mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
    else:
        mean, var = rs[0].double(), rs[1].double()
    sc = g1.double() / torch.sqrt(var + 1e-5)
    b1 = (sc * (mean - (torch.round(mean * 4096) + 0.5) / 4096)).float()
    deg = torch.bincount((idx + torch.arange(B).view(B, 1, 1) * N).view(-1), minlength=P)
    return Inputs(B, N, k, slope, training, xp, idx, W1, g1, b1, W2, g2, b2, rs, w, deg == 0)


def reference(inp, sel=None, dtype=torch.float64, split_centre=False):
    """The restatement and its gradients for `inp` in `dtype`, the max over k taking the slots `sel` [P, 128] (None: its own).
    -> dict: out, the seven gradients, the running statistics after the call (momentum 0.1; the given ones in eval mode), the parts of
    tnet_edge_f64 (detached), bn1_scale [64]; split_centre: also dx_nbr and dx_ctr, the neighbour and centre shares of dx."""
    leaves = [t.detach().to(dtype, copy=True).requires_grad_(True) for t in (inp.xp, inp.W1, inp.g1, inp.b1, inp.W2, inp.g2, inp.b2)]
    rs = [t.to(dtype) for t in inp.rs]
    xc = leaves[0].detach().clone().requires_grad_(True) if split_centre else None
    out, parts = tnet_edge_f64(leaves[0], inp.idx, *leaves[1:], inp.slope, sel=sel, stats=None if inp.training else rs, parts=True, xc=xc)
    out.backward(inp.w.to(dtype))
    res = dict(zip(GRADS, (t.grad for t in leaves)), out=out.detach(), **{n: t.detach() for n, t in parts.items()})
    if split_centre:
        res.update(dx_nbr=leaves[0].grad, dx_ctr=xc.grad, dx=leaves[0].grad + xc.grad)
    E = inp.B * inp.N * inp.k
    for i, n in enumerate(("y", "z")):
        if inp.training:
            t = res[n]
            rs[2 * i] = 0.9 * rs[2 * i] + 0.1 * t.mean((0, 2, 3))
            rs[2 * i + 1] = 0.9 * rs[2 * i + 1] + 0.1 * t.var((0, 2, 3), unbiased=False) * E / (E - 1)
    res.update(zip(STATS, rs))
    var1 = res["y"].var((0, 2, 3), unbiased=False) if inp.training else inp.rs[1].to(dtype)
    res["bn1_scale"] = leaves[2].detach() / torch.sqrt(var1 + 1e-5)
    return res


def kink_margins(inp, ref=None):
    """-> (the smallest |first-layer pre-activation| over all edges in units of the BN1 scale, the smallest |second-layer pre-activation|
    at the slot the float64 arg-max / arg-min of z picks) of the float64 restatement"""
    ref = ref or reference(inp)
    m1 = (ref["a1"] / ref["bn1_scale"].view(1, -1, 1, 1)).abs().min().item()
    # BN2 is monotone per channel (rising for gamma2 >= 0, falling otherwise): the extreme of z is the maximum of a2
    m2 = ref["a2"].max(dim=-1)[0].abs().min().item()
    return m1, m2


# ----------------------------------------------------------------------------- the case table of tests/test_gpu_tnet.py
# name -> (B, N, k, mode, options, seed): options go to dyadic_case (slope, training, graph, neg) except `xgrad` (False: x takes no
# gradient).  N leaves the last tile of every cloud partial wherever a tile holds more than one point.  Seeds: the first for which
# conditions (b) and (c) of tests/test_tnet_restatement_cpu.py hold (`PYTHONPATH=. python tests/tnet_restatement.py` searches and prints them).
Case = collections.namedtuple("Case", "name B N k mode opt fwd bwd")
CASES = collections.OrderedDict()
SEEDS = {}                  # input_key -> seed


def _case(name, B, N, k, mode, fwd, bwd, **opt):
    assert name not in CASES
    CASES[name] = Case(name, B, N, k, mode, opt, fwd, bwd)


def _n(k):
    """a cloud size whose last tile is partial in every kernel that tiles k (and N > k for the kNN graph)"""
    for N in range(max(45, k + 2), 400):
        if all(N % t for t in {points_per_tile(k), points_per_tile(k, True)} if t > 1):
            return N


# every tnet_edge_bwdg_kernel instantiation, at the first and last k of its range (mode fp32, slope 0.2); one odd k in the default mode
for _k, _kern in ((3, "<0,20>"), (13, "<0,20>"), (20, "<0,20>"), (21, "<0,24>"), (24, "<0,24>"), (25, "<0,32>"), (32, "<0,32>"), (33, "<1,40>"),
                  (40, "<1,40>"), (41, "<2,32>"), (64, "<2,32>"), (65, "<2,32>"), (96, "<2,32>"), (97, "<2,32>"), (128, "<2,32>")):
    _case("bwdg-k%d" % _k, 2, _n(_k), _k, "fp32", "fwd2<%d>" % _k if _k in (20, 40) else "fwd", "bwdg" + _kern)
_case("bwdg-k13-default", 2, _n(13), 13, "default", "fwd", "bwdg<0,20>")
# tnet_edge_bwds_kernel, three products and one
for _k in (8, 10, 24, 32, 48, 64):
    _case("bwds-k%d" % _k, 2, _n(_k), _k, "f16x3", "fwd", "bwds")
    _case("bwds-k%d-bf16" % _k, 2, _n(_k), _k, "bf16", "fwd", "bwds<ONEP>")
# the round-1 kernel (slope = 0)
for _k, _mode in ((7, "fp32"), (24, "f16x3"), (64, "fp32"), (100, "bf16x6")):
    _case("bwd-k%d" % _k, 2, _n(_k), _k, _mode, "fwd", "bwd", slope=0.0)
# the forward kernels on a partial last tile: 2 of 8 points (k = 20, N = 50), 2 of 4 (k = 40, N = 42)
for _k, _N in ((20, 50), (40, 42)):
    for _mode in ("fp32", "bf16x6", "f16x3", "bf16"):
        _case("fwd-k%d-%s" % (_k, _mode), 2, _N, _k, _mode, fwd_kernel(_k, _mode), bwd_kernel(_k, _mode, 0.2))
for _k in (1, 5, 64, 65, 128):
    for _mode in ("fp32", "f16x3"):
        _case("fwd-k%d-%s" % (_k, _mode), 2, _n(_k), _k, _mode, "fwd", bwd_kernel(_k, _mode, 0.2))
# the persistent tile walk, more tiles than workgroups: 5 points per tile at k = 24; B = 8 takes the XCD-aware walk, B = 3 the plain one
_case("walk-gram-xcd", 8, 165, 24, "fp32", "fwd", "bwdg<0,24>")          # 264 tiles on 256 workgroups
_case("walk-gram-plain", 3, 428, 24, "fp32", "fwd", "bwdg<0,24>")        # 258 on 256
_case("walk-fwd-xcd", 8, 330, 24, "fp32", "fwd", "bwdg<0,24>")           # 528 on 512 (forward); 528 on 256 (backward)
_case("walk-fwd-plain", 3, 853, 24, "fp32", "fwd", "bwdg<0,24>")         # 513 on 512
# forced indices: degree-0 points, a hub, repeated entries; with a gradient on x (tnet_edge_bwd2_kernel) and without (the moment pass)
for _k, _mode, _kern in ((16, "f16x3", "bwds"), (24, "fp32", "bwdg<0,24>")):
    for _xg in (True, False):
        _case("forced-k%d-%s" % (_k, "dx" if _xg else "nodx"), 2, 64, _k, _mode, "fwd", _kern, graph="forced", xgrad=_xg)
# a quarter of the BatchNorm scales negative: zsel is a minimum there, BN1's slope recovery divides by a negative scale
_case("neg-bwds", 2, 52, 24, "f16x3", "fwd", "bwds", neg=True)
_case("neg-bwdg", 2, 50, 32, "fp32", "fwd", "bwdg<0,32>", neg=True)
_case("neg-bwd", 2, 52, 24, "fp32", "fwd", "bwd", neg=True, slope=0.0)
# eval mode: the given running statistics
_case("eval-bwds", 2, 45, 10, "f16x3", "fwd", "bwds", training=False)
_case("eval-bwdg", 2, 50, 33, "fp32", "fwd", "bwdg<1,40>", training=False)
_case("eval-bwd", 2, 45, 7, "fp32", "fwd", "bwd", training=False, slope=0.0)
# a small slope: the Gram forms recover the pre-activation by dividing by it
_case("slope-bwds", 2, 50, 32, "f16x3", "fwd", "bwds", slope=0.01)
_case("slope-bwdg", 2, 50, 20, "fp32", "fwd2<20>", "bwdg<0,20>", slope=0.01)
# run to run
_case("repro-bwdg", 2, 100, 96, "fp32", "fwd", "bwdg<2,32>")
_case("repro-bwds", 2, 51, 48, "f16x3", "fwd", "bwds")

SEEDS.update({(8, 165, 24, 0.2, True, "knn", False): 2, (3, 428, 24, 0.2, True, "knn", False): 2, (8, 330, 24, 0.2, True, "knn", False): 10,
              (3, 853, 24, 0.2, True, "knn", False): 5, (2, 52, 24, 0.0, True, "knn", True): 1})          # every other case: seed 0

_inputs = {}


def input_key(c):
    o = c.opt
    return (c.B, c.N, c.k, o.get("slope", 0.2), o.get("training", True), o.get("graph", "knn"), o.get("neg", False))


def case_inputs(name, seed=None):
    """the Inputs of CASES[name], built once per distinct (shape, options): cases that differ in the product mode only share them"""
    c = CASES[name]
    key = input_key(c)
    if seed is not None:
        return dyadic_case(*key[:3], seed, *key[3:])
    if key not in _inputs:
        _inputs[key] = dyadic_case(*key[:3], SEEDS.get(key, 0), *key[3:])
    return _inputs[key]


def find_seed(key, limit=200):
    """the first seed whose inputs keep both kink margins"""
    for seed in range(limit):
        m1, m2 = kink_margins(dyadic_case(*key[:3], seed, *key[3:]))
        if m1 >= 0.999 * KINK1 and m2 >= KINK2:
            return seed
    raise RuntimeError("no seed below %d for %r" % (limit, key))


if __name__ == "__main__":
    for key in dict.fromkeys(input_key(c) for c in CASES.values()):
        print("    %r: %d," % (key, find_seed(key)), flush=True)
