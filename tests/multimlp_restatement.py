"""Own-words torch restatement of the heads' merged layers (mlsp_amd/csrc/multi.hip, Fh.multimlp / Fh.pointmlp with chain=True),
parameterised by dtype: the float64 yardstick of tests/test_gpu_multimlp.py and, in fp32 on the CPU, the stand-in for fp32 rounding.
Plain torch ops only; runs anywhere.

One layer: several Linear (+bias) layers side by side on column slices of X, ONE BatchNorm over all their output channels, then a
per-channel activation and dropout.  Written as  z = a * g  with  a = gamma (y - mean) / sqrt(var + eps) + beta  and g a CONSTANT
matrix, the gate: g = 0 where the element is off, else (a > 0 ? 1 : slope_c) * (dropout channel ? 256 / (256 - t) : 1) with
t = min(255, int(256 p + 0.5)) -- the byte threshold of csrc/common.h (dropout_thresh8 / dropout_inv_keep8).  Autograd through a * g
is the exact gradient for that gate.  The gate of a run under test is read off that run (gate_from_z, gate_from_preact); `admissible`
counts what a test must bound so that a wrong kernel cannot buy itself a wrong gate.

`spec` = ((Cout, negative-side factor, dropout on), ...) per segment, as Fh.channel_params takes it (factor 0 = ReLU, 0.2 =
LeakyReLU(0.2), 1 = no activation).  `segs` = [(x_col, W [Cout, Cin], bias | None), ...]."""
import math

import torch

EPS = 1e-5


def dist(a, b):
    """max|a - b| / max|b|"""
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max()).item()


def thresh(p):
    return min(255, int(256 * p + 0.5)) if p > 0 else 0


def inv_keep(p):
    t = thresh(p)
    return 256.0 / (256 - t) if t else 1.0


def channels(spec, dtype=torch.float64):
    """-> (slope [C], dropout switch [C] bool)"""
    sl = torch.cat([torch.full((c,), float(f), dtype=dtype) for c, f, _ in spec])
    dr = torch.cat([torch.full((c,), bool(d)) for c, _, d in spec])
    return sl, dr


def _factors(spec, p, dtype):
    """-> (positive-side factor [C], negative-side factor [C], dropout switch [C]) of the elements that are on"""
    sl, dr = channels(spec, dtype)
    pos = torch.where(dr, torch.full_like(sl, inv_keep(p)), torch.ones_like(sl))
    return pos, sl * pos, dr & (thresh(p) > 0)


def act_gate(a, spec, keep=None, p=0.0):
    """the gate a run of the layer itself would use: the activation side by the sign of `a`, dropout by `keep` ([M, C] bool; read on
    the dropout channels only, None: nothing dropped)"""
    pos, neg, dr = _factors(spec, p if keep is not None else 0.0, a.dtype)
    g = torch.where(a > 0, pos, neg).expand_as(a)
    if keep is not None:
        g = torch.where(keep | ~dr, g, torch.zeros_like(g))
    return g


def gate_from_z(Z, spec, p, dtype=torch.float64):
    """The gate of a materialised layer from its output alone.  Z > 0: the positive-side factor; Z < 0: the negative-side one.  Z == 0:
    on a dropout channel or behind a ReLU the element is off -- ReLU-off and dropped are indistinguishable there and equivalent, value 0
    and gradient 0 either way; elsewhere a == 0 exactly and the kernel's derivative is the negative side's (`!(a > 0)`)."""
    pos, neg, dr = _factors(spec, p, dtype)
    Z = Z.to(dtype)
    zero = torch.where(dr, torch.zeros_like(neg), neg)
    return torch.where(Z > 0, pos, torch.where(Z < 0, neg, zero))


def keep_from_z(Z, spec):
    """[M, C] bool: False where a dropout channel's element of a materialised layer is off (dropped, or behind a ReLU that is off --
    which leaves nothing to keep), True elsewhere"""
    _, dr = channels(spec)
    return (Z != 0) | ~dr


def gate_from_preact(y, bn_save, spec, keep, p, dtype=torch.float64):
    """The gate of a deferred layer (no Z exists): the activation side from the run's own pre-BatchNorm output y [M, C] and
    bn_save [4, C] (scale | shift | ..) as the sign of y * scale + shift evaluated in float64 -- the product of two fp32 numbers is
    exact there and the rounding of a sum never changes its sign, so this is the sign of the kernel's fmaf(y, scale, shift); dropout
    from `keep` (keep_from_z of a materialised run with the same dropout stream)."""
    a = y.double() * bn_save[0].double() + bn_save[1].double()
    return act_gate(a, spec, keep, p).to(dtype)


def admissible(gate, a64, spec, p):
    """What bounds a gate taken from a run under test, against the float64 BatchNorm output a64 [M, C] of the reference:
    n              elements
    tau            1e-5 x max|a64|
    bad_values     elements whose gate is none of 0 / positive-side factor / negative-side factor of their channel
    illegal_off    gate 0 on a channel without dropout whose negative-side factor is not 0
    contradictions elements that are on with the side the sign of a64 contradicts, or off on a channel without dropout where a64 > 0
    contra_max     max|a64| over those (0 without any)
    eligible, kept on the dropout channels: elements whose float64 activation exceeds tau in magnitude, and how many of them are on
    keep_sigma     |kept - eligible q| / sqrt(eligible q (1 - q)), q = 1 - t / 256
    keep_sigma_channel  the largest of the same per channel"""
    pos, neg, dr = _factors(spec, p, torch.float64)
    g, a = gate.double(), a64.double()
    tau = 1e-5 * a.abs().max().item()
    on = g != 0
    is_pos, is_neg = on & (g == pos), on & (g == neg)
    out = {"n": g.numel(), "tau": tau}
    out["bad_values"] = int((on & ~is_pos & ~is_neg).sum())
    out["illegal_off"] = int((~on & ~dr & (neg != 0)).sum())
    same = (pos == neg).expand_as(g)                        # no activation: the side does not show
    contra = ((is_pos & ~is_neg & (a <= 0)) | (is_neg & ~is_pos & (a > 0))) & ~same
    contra = contra | (~on & ~dr & (a > 0))                 # off without dropout: only a non-positive activation (behind a ReLU) does that
    out["contradictions"] = int(contra.sum())
    out["contra_max"] = a.abs()[contra].max().item() if out["contradictions"] else 0.0
    act = torch.where(a > 0, a, a * (neg / pos))            # the float64 activation
    elig = (act.abs() > tau) & dr
    q = 1.0 - thresh(p) / 256.0
    n_c, k_c = elig.sum(0).double(), (elig & on).sum(0).double()
    out["eligible"], out["kept"] = int(n_c.sum()), int(k_c.sum())

    def sigma(k, n):
        return abs(k - n * q) / math.sqrt(n * q * (1 - q)) if n > 0 and 0 < q < 1 else (0.0 if k == n * q else math.inf)
    out["keep_sigma"] = sigma(out["kept"], out["eligible"])
    out["keep_sigma_channel"] = max([sigma(k, n) for k, n, d in zip(k_c.tolist(), n_c.tolist(), dr.tolist()) if d] or [0.0])
    return out


def layer(X, segs, gamma, beta, run_mean, run_var, gate, training=True, momentum=0.1, eps=EPS, dtype=torch.float64, tap=None):
    """-> (z, y, mean, var_biased, new_run_mean, new_run_var).  `gate`: [M, C] constant, or a callable a -> gate (act_gate).  Batch
    statistics over the M rows in training (the running variance takes the unbiased one), the running statistics in eval (returned as
    mean / var, and unchanged).  `tap` (a list): the BatchNorm output a (detached) and the gate used are appended.  Tensors that require
    grad keep doing so."""
    X = X.to(dtype)
    y = torch.cat([X[:, xc:xc + W.shape[1]] @ W.to(dtype).t() + (0 if b is None else b.to(dtype)) for xc, W, b in segs], dim=1)
    M = y.shape[0]
    rm = None if run_mean is None else run_mean.detach().to(dtype)
    rv = None if run_var is None else run_var.detach().to(dtype)
    if training:
        mean = y.mean(0)
        var = ((y - mean) ** 2).mean(0)
        new_rm = None if rm is None else (1 - momentum) * rm + momentum * mean.detach()
        new_rv = None if rv is None else (1 - momentum) * rv + momentum * var.detach() * (M / (M - 1))
    else:
        mean, var, new_rm, new_rv = rm, rv, rm, rv
    a = gamma.to(dtype) * (y - mean) / torch.sqrt(var + eps) + beta.to(dtype)
    g = gate(a.detach()) if callable(gate) else gate.to(dtype)
    if tap is not None:
        tap.append((a.detach(), g))
    return a * g, y, mean, var, new_rm, new_rv


def layer_grads(X, segs, gamma, beta, run_mean, run_var, gate, R, training=True, dtype=torch.float64, x_grad=True, tap=None):
    """name -> tensor of one layer's forward and the backward of (z * R).sum(): Z, Y, mean, var, run_mean, run_var, dX, dW<i>, db<i>,
    dgamma, dbeta (inputs are detached first)"""
    X = X.detach().clone().requires_grad_(x_grad)
    segs = [(xc, W.detach().clone().requires_grad_(True), None if b is None else b.detach().clone().requires_grad_(True)) for xc, W, b in segs]
    gamma, beta = (t.detach().clone().requires_grad_(True) for t in (gamma, beta))
    z, y, mean, var, rm, rv = layer(X, segs, gamma, beta, run_mean, run_var, gate, training, dtype=dtype, tap=tap)
    (z * R.to(dtype)).sum().backward()
    q = {"Z": z.detach(), "Y": y.detach(), "mean": mean.detach(), "var": var.detach(), "dgamma": gamma.grad, "dbeta": beta.grad}
    if rm is not None:
        q["run_mean"], q["run_var"] = rm, rv
    if x_grad:
        q["dX"] = X.grad
    for i, (_, W, b) in enumerate(segs):
        q["dW%d" % i] = W.grad
        if b is not None:
            q["db%d" % i] = b.grad
    return q


# ---- the head stack (PointDA/Models.py:192-197, 226-231, 272-285) as the model runs it ----------------------------------------------
C0 = 512
P_DROP = 0.5
SPEC_IN = ((1024, 0.0, True),)
SPEC0 = ((256, 0.0, True), (256, 0.0, True), (256, 0.2, True))
SPEC1 = ((128, 0.0, False), (128, 0.0, False), (256, 0.2, True))
SPECS = (SPEC_IN, SPEC0, SPEC1)
SEG0 = ((0, 256, 256, False), (256, 256, 256, False), (512, 512, 256, True))         # (x_col, Cin, Cout, bias)
SEG1 = ((0, 256, 128, False), (256, 256, 128, False), (512, 256, 256, True))
FIN = ((0, 128, 3, False), (128, 128, 3, False), (256, 256, 16, True))
STAT_NAMES = ("rm0", "rv0", "rm1", "rv1", "rm2", "rv2")


def head_params(M, seed=5):
    """the parameters of test_merged_layers_deferred_activation_chain: uniform in [-1, 1], weights scaled by 0.1 (0.2 in the final
    layers); name -> fp32 tensor, X and the three loss weights R0..R2 included"""
    g = torch.Generator().manual_seed(seed)

    def r(*shape, s=1.0):
        return (torch.rand(shape, generator=g) * 2 - 1) * s
    p = {"X": r(M, C0), "W1": r(1024, C0, s=0.1), "g1": r(1024), "b1": r(1024)}
    for d, segs in (("d0", SEG0), ("d1", SEG1)):
        for i, (_, ci, co, hb) in enumerate(segs):
            p["%s.W%d" % (d, i)] = r(co, ci, s=0.1)
            if hb:
                p["%s.b%d" % (d, i)] = r(co)
    p["gb0.gamma"], p["gb0.beta"], p["gb1.gamma"], p["gb1.beta"] = r(768), r(768), r(512), r(512)
    for i, (_, ci, co, hb) in enumerate(FIN):
        p["fin.W%d" % i] = r(co, ci, s=0.2)
        if hb:
            p["fin.b%d" % i] = r(co)
    for i, (_, _, co, _) in enumerate(FIN):
        p["R%d" % i] = torch.randn(M, co, generator=g)
    return p


LEAVES = tuple(k for k in head_params(2) if not k.startswith("R"))


def fresh_stats(dtype=torch.float32, device=None):
    return [(torch.zeros if i % 2 == 0 else torch.ones)(c, dtype=dtype, device=device) for c in (1024, 768, 512) for i in range(2)]


def _segs(p, d, segs):
    return [(xc, p["%s.W%d" % (d, i)], p.get("%s.b%d" % (d, i))) for i, (xc, _, _, _) in enumerate(segs)]


def head_stack(params, X, gates, dtype=torch.float64, training=True, stats=None, tap=None):
    """pointmlp 512 -> 1024 (ReLU, p 0.5), multimlp SPEC0, multimlp SPEC1, the three final Linear layers on column slices.
    gates: one per BatchNorm layer (constants or callables).  -> (outs [3], new running statistics [6])"""
    p = params
    st = fresh_stats(dtype) if stats is None else stats
    h, _, _, _, rm0, rv0 = layer(X, [(0, p["W1"], None)], p["g1"], p["b1"], st[0], st[1], gates[0], training, dtype=dtype, tap=tap)
    h, _, _, _, rm1, rv1 = layer(h, _segs(p, "d0", SEG0), p["gb0.gamma"], p["gb0.beta"], st[2], st[3], gates[1], training, dtype=dtype, tap=tap)
    h, _, _, _, rm2, rv2 = layer(h, _segs(p, "d1", SEG1), p["gb1.gamma"], p["gb1.beta"], st[4], st[5], gates[2], training, dtype=dtype, tap=tap)
    outs = [h[:, xc:xc + W.shape[1]] @ W.to(dtype).t() + (0 if b is None else b.to(dtype)) for xc, W, b in _segs(p, "fin", FIN)]
    return outs, [rm0, rv0, rm1, rv1, rm2, rv2]


def grads(params, gates, dtype=torch.float64, weights=(1.0, 1.0, 1.0), training=True, tap=None):
    """name -> tensor: out0..2, "d <leaf>" for every leaf (X included) of the loss sum_i weights[i] (out_i * R_i).sum(), and the six
    running statistics after the step.  A leaf the loss does not reach has a zero gradient."""
    p = {k: (v.detach().clone().requires_grad_(True) if k in LEAVES else v) for k, v in params.items()}
    outs, stats = head_stack(p, p["X"], gates, dtype, training, tap=tap)
    loss = sum(w * (o * p["R%d" % i].to(dtype)).sum() for i, (o, w) in enumerate(zip(outs, weights)) if w)
    loss.backward()
    q = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
    for k in LEAVES:
        q["d " + k] = p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])
    q.update(zip(STAT_NAMES, stats))
    return q


# ---- the cases of tests/test_gpu_multimlp.py (tier 1) ---------------------------------------------------------------------------------
# One merged layer per case: segments (x_col, Cin, Cout, bias, negative-side factor, dropout on).  Beside each: the branch of
# csrc/multi.hip it reaches, derived from multi_check / multi_group_run (multi.hip), gemm_pick_split / gemm_pick_bm (gemm.hip; 128 x 128
# tiles, 32-deep K-tiles: K splits when there are < 256 tiles and >= 4 K-tiles, into min(ceil(512 / tiles), K-tiles / 2) parts) and
# multi_rows_per_block (tpr = Ctot / 4 threads per row, nrg = 256 / tpr row groups).
MODEL_SEGS = ((0, 256, 256, False, 0.0, True), (256, 256, 256, False, 0.0, True), (512, 512, 256, True, 0.2, True))
MIXED_SEGS = ((0, 128, 128, False, 0.0, True), (128, 128, 128, False, 0.0, True), (256, 64, 36, True, 0.2, True))
EPI_SEGS = ((0, 64, 128, False, 0.0, True), (64, 64, 128, False, 0.2, False), (128, 96, 64, True, 1.0, True))
TIER1 = {
    # smallest legal M (multi_check refuses M <= 32), K = 8 / 16: one K-tile, no split, 128-row panels (M < 256): statistics out of the
    # GEMM epilogues, one ragged panel.  Ctot 12: tpr 3, nrg 85, thread 255 idle; 33 rows < nrg: a ragged first row group
    "m33": dict(M=33, ldx=24, segs=((0, 8, 4, False, 0.0, True), (8, 16, 8, True, 0.2, False)), seed=11),
    # segments 0 / 1: no bias, Cin = Cout = 128, M % 128 == 0, back to back: ONE block-diagonal launch [256 x 256 x 128]: 4 tiles,
    # 4 K-tiles -> 2 K splits, no epilogue statistics; segment 2: K = 64, 2 K-tiles, no split -> mixed: launch_colstats_n for all.
    # Ctot 292: tpr 73, nrg 3, 37 threads idle
    "m256_mixed": dict(M=256, ldx=320, segs=MIXED_SEGS, seed=12),
    # every K < 128 (2 / 2 / 3 K-tiles): no split; Cin % 128 != 0: no block-diagonal launch; M = 256: 2 tiles < 1536 and M >= 256 -> 64-row
    # panels, 4 partial rows out of the epilogues.  Segment 2: no activation (factor 1) under dropout.  Ctot 320: tpr 80, nrg 3
    "m256_epilogue": dict(M=256, ldx=224, segs=EPI_SEGS, seed=13),
    # the same at M = 200 < 256: 128-row panels, one full and one ragged (72 rows)
    "m200_epilogue": dict(M=200, ldx=224, segs=EPI_SEGS, seed=14),
    # Ctot 1024, the cap of multi_check: tpr 256, nrg 1 (every thread one quad of one row, 4 rows per workgroup step); K = 32: one K-tile,
    # panels of 128 + 2 rows
    "m130_ctot1024": dict(M=130, ldx=64, segs=((0, 32, 512, False, 0.0, False), (32, 32, 512, True, 0.2, True)), seed=15),
    # the model's spec.  M = 1100: M % 128 != 0 -> three single launches, ragged last tile row (76 rows); [1100 x 256 x 256]: 18 tiles,
    # 8 K-tiles -> 4 splits, [.. x 512]: 16 K-tiles -> 8 splits: statistics by launch_colstats_n.  p = 0.3: t = 77, 256 / 179
    "model_m1100": dict(M=1100, ldx=1024, segs=MODEL_SEGS, p=0.3, seed=16),
    # M = 2048: block-diagonal launch of segments 0 / 1 [2048 x 512 x 256]: 64 tiles, 8 K-tiles -> 4 splits; segment 2: 32 tiles,
    # 16 K-tiles -> 8 splits
    "model_m2048": dict(M=2048, ldx=1024, segs=MODEL_SEGS, p=0.3, seed=17),
    # eval: nothing dropped, scale / shift from the running statistics (launch_bn_eval_prepare), which stay; dbias by launch_colsum
    "m256_mixed_eval": dict(M=256, ldx=320, segs=MIXED_SEGS, training=False, seed=18),
    "model_m1100_eval": dict(M=1100, ldx=1024, segs=MODEL_SEGS, training=False, seed=19),
    # both segments read columns 0..127: the second dgrad ACCUMULATES into dX (`acc`); Cout 64: no block-diagonal launch; forward
    # [256 x 64 x 128]: 2 tiles, 4 K-tiles -> 2 splits; dgrad [256 x 128 x 64]: 2 K-tiles, no split
    "m256_shared_input": dict(M=256, ldx=128, segs=((0, 128, 64, False, 0.0, True), (0, 128, 64, True, 0.2, False)), seed=20),
    # partially overlapping inputs: legal forward, no input gradient (dX == NULL)
    "m256_overlap_no_dx": dict(M=256, ldx=192, segs=((0, 128, 64, False, 0.0, True), (64, 128, 64, True, 0.2, False)), x_grad=False, seed=21),
    # "m256_mixed" with negative scales, one scale exactly zero and an all-zero weight row (a constant column: variance exactly 0)
    "m256_channel_edges": dict(M=256, ldx=320, segs=MIXED_SEGS, edges=True, seed=22),
}
ZERO_ROW, ZERO_GAMMA = 7, 133           # channels of "m256_channel_edges"
CHAIN_M = (1100, 2048)


def spec_of(case):
    return tuple((co, sl, dr) for _, _, co, _, sl, dr in case["segs"])


def make_case(name):
    """the inputs of a TIER1 case: uniform in [-1, 1], weights and biases scaled by 0.1 (a bias of the size of the column's spread: no
    column is off-centre, |mean| >> std, which is another subject), gamma = U(-1, 1) + 0.3 (negative scales included)"""
    c = dict(TIER1[name])
    c.setdefault("p", 0.5)
    c.setdefault("training", True)
    c.setdefault("x_grad", True)
    g = torch.Generator().manual_seed(c["seed"])

    def r(*shape, s=1.0):
        return (torch.rand(shape, generator=g) * 2 - 1) * s
    c["X"] = r(c["M"], c["ldx"])
    c["W"] = [r(co, ci, s=0.1) for _, ci, co, _, _, _ in c["segs"]]
    c["b"] = [r(co, s=0.1) if hb else None for _, _, co, hb, _, _ in c["segs"]]
    C = sum(co for _, _, co, _, _, _ in c["segs"])
    c["gamma"], c["beta"] = r(C) + 0.3, r(C)
    c["run_mean"], c["run_var"] = r(C, s=0.1), torch.rand(C, generator=g) + 0.5
    c["R"] = torch.randn(c["M"], C, generator=g)
    if c.get("edges"):
        c["W"][0][ZERO_ROW] = 0
        c["beta"][ZERO_ROW] = 0.37
        c["gamma"][ZERO_GAMMA] = 0
        c["gamma"][:4] = -c["gamma"][:4].abs() - 0.1
    c["spec"] = spec_of(c)
    c["rs_segs"] = [(sg[0], W, b) for sg, W, b in zip(c["segs"], c["W"], c["b"])]
    return c


def is_bias_grad(name):
    return name[:2] == "db" and name[2:].isdigit()


def random_keep(shape, p, seed):
    """a keep mask of the kernels' rate: a byte per element, kept iff byte >= t"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=g) >= thresh(p)


def case_grads(c, gate, dtype, tap=None):
    return layer_grads(c["X"], c["rs_segs"], c["gamma"], c["beta"], c["run_mean"], c["run_var"], gate, c["R"], c["training"], dtype,
                          x_grad=c["x_grad"], tap=tap)


def assert_admissible(a, M, zero_contradictions=False):
    assert a["bad_values"] == 0 and a["illegal_off"] == 0, a
    assert a["contradictions"] <= (0 if zero_contradictions else 1e-5 * a["n"]) and a["contra_max"] <= a["tau"], a
    assert a["keep_sigma"] <= 5, a
    if M >= 256:
        assert a["keep_sigma_channel"] <= 6, a
