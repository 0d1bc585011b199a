"""Float64 restatements of the five operations of csrc/loss.hip, and the seeded cases of tests/test_gpu_losses.py.  CPU only.

The references are oracle/ref_cpu.py (chamfer_distance, reconstruction_loss, normal_prediction_loss, densityloss) run in float64 under
autograd, torch.softmax and (p * w).sum(1) for the cardinality tail.  ref_cpu's Chamfer materialises [B, N, N, 3]; the masked-row form
below evaluates only the masked rows of p1 against all columns of p2 -- the unmasked rows are multiplied by zero in the reference, so
value and gradients are the same (tests/test_loss_restatement_cpu.py checks that wherever both fit) -- and takes the FIRST minimum
explicitly, which is what the kernels promise on exact ties.

dist(a, b) = max|a - b| / max|b|.  Yardstick of a quantity: dist from float64 of the same reference run in fp32 on the CPU.
Bar: min(1e-4, max(2e-6, 3 x yardstick)) -- 2e-6 the GEMM family's floor, 3 for the differing summation order, 1e-4 today's golden
tolerance as a cap."""
import types

import torch

from oracle import ref_cpu

FLOOR, CAP, GAP_MIN, YARD_MAX = 2e-6, 1e-4, 1e-3, 3e-5
REF_CPU_MAX_N = 1639      # beyond it the fp32 yardstick is the masked-row form too: ref_cpu's [B, N, N, 3] tensors take seconds and, at N = 6400, gigabytes


def dist(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    den = b.abs().max().item() if b.numel() else 0.0
    return (a - b).abs().max().item() / den if den > 0 else (a - b).abs().max().item()


def bar(yard):
    return min(CAP, max(FLOOR, 3 * yard))


# --------------------------------------------------------------------------------------------- Chamfer
def _penalty(mc):
    return torch.where(mc == 0, torch.full_like(mc, 100.0), torch.zeros_like(mc))


def _row_table(p1b, p2b, mcb):
    """-> (masked row indices [R], d [R, N]) of one cloud: d = |p1_i - p2_j|^2 (sqrt, then squared, as the reference) + penalty_j"""
    rows = torch.nonzero(mcb != 0).reshape(-1)
    d = torch.norm(p1b[rows].unsqueeze(1) - p2b.unsqueeze(0), 2, dim=2) ** 2 + _penalty(mcb).unsqueeze(0)
    return rows, d


def _first_min(d):
    """lowest arg-min column of every row of d [R, N]"""
    N = d.shape[1]
    col = torch.arange(N).unsqueeze(0).expand_as(d)
    return torch.where(d == d.min(dim=1, keepdim=True)[0], col, torch.full_like(col, N)).min(dim=1)[0]


def chamfer_dir_rows(p1, p2, mc):
    """ref_cpu.chamfer_distance(p1, p2, mask) with mc = mask[:, :, 0], over the masked rows only, first minimum on ties"""
    total = 0
    for b in range(p1.shape[0]):
        rows, d = _row_table(p1[b], p2[b], mc[b])
        if rows.numel() == 0:
            total = total + (p1[b].sum() * 0 + p2[b].sum() * 0) / mc[b].sum()          # 0 / 0 as the reference
            continue
        dmin = d.gather(1, _first_min(d.detach()).unsqueeze(1)).squeeze(1)
        total = total + (dmin * mc[b][rows]).sum() / mc[b].sum()
    return total


def reconstruction_rows(pred, gold, mask):
    """ref_cpu.reconstruction_loss in the masked-row form.  pred [B,N,3]; gold, mask [B,3,N]"""
    gt, mc = gold.permute(0, 2, 1), mask[:, 0, :]
    return (chamfer_dir_rows(gt, pred, mc) + chamfer_dir_rows(pred, gt, mc)) / pred.shape[0]


def selection(p1, p2, mc):
    """-> (arg [B, N] int64: first arg-min column of every masked row, -1 elsewhere;  gap [B, N]: (second - best) / second of the
    row's distances, inf where there is no second column and on unmasked rows).  Evaluated in the dtype of p1."""
    B, N = mc.shape
    arg = torch.full((B, N), -1, dtype=torch.int64)
    gap = torch.full((B, N), float("inf"), dtype=torch.float64)
    for b in range(B):
        rows, d = _row_table(p1[b], p2[b], mc[b])
        if rows.numel() == 0:
            continue
        a = _first_min(d)
        arg[b, rows] = a
        if N > 1:
            best = d.gather(1, a.unsqueeze(1)).squeeze(1)
            second = d.scatter(1, a.unsqueeze(1), float("inf")).min(dim=1)[0]
            gap[b, rows] = ((second - best) / second).double()
    return arg, gap


def _leaf(t, dtype):
    return t.detach().to(dtype).clone().requires_grad_(True)


def fused_reference(case, dtype=torch.float64, form="rows"):
    """-> dict(loss, d_pred) of reconstruction_loss; form "rows" (masked-row form) or "ref_cpu" """
    pred = _leaf(case.pred, dtype)
    gold, mask = case.gold.to(dtype), case.mask.to(dtype)
    loss = (reconstruction_rows if form == "rows" else ref_cpu.reconstruction_loss)(pred, gold, mask)
    loss.backward()
    return dict(loss=loss.detach(), d_pred=pred.grad)


def dir_reference(case, dtype=torch.float64, form="rows"):
    """-> dict(loss, d_p1, d_p2) of chamfer_distance(pred, gold^T, mask^T)"""
    p1, p2 = _leaf(case.pred, dtype), _leaf(case.gold.permute(0, 2, 1).contiguous(), dtype)
    m3 = case.mask.permute(0, 2, 1).to(dtype)
    loss = chamfer_dir_rows(p1, p2, m3[:, :, 0]) if form == "rows" else ref_cpu.chamfer_distance(p1, p2, m3)
    loss.backward()
    return dict(loss=loss.detach(), d_p1=p1.grad, d_p2=p2.grad)


def fp32_form(N):
    """which form serves as the fp32 yardstick at this N"""
    return "ref_cpu" if N <= REF_CPU_MAX_N else "rows"


def _case(name, pred, gold, mask1, ties=False):
    """pred [B,N,3], gold [B,3,N], mask1 [B,N] 0/1 -> case with mask [B,3,N] (as deform_input returns it)"""
    mask = mask1[:, None, :].repeat(1, 3, 1).contiguous().float()
    return types.SimpleNamespace(name=name, pred=pred.float().contiguous(), gold=gold.float().contiguous(), mask=mask,
                                 B=pred.shape[0], N=pred.shape[1], ties=ties)


def _clouds(g, B, N, noise=0.05):
    """gold [B,3,N] = a cloud in [-1, 1]^3 plus noise, pred [B,N,3] = the same cloud plus other noise (golden_common.make_inputs)"""
    x = torch.rand(B, 3, N, generator=g) * 2 - 1
    gold = x + noise * torch.randn(B, 3, N, generator=g)
    pred = (x + noise * torch.randn(B, 3, N, generator=g)).permute(0, 2, 1).contiguous()
    return pred, gold


def _random_mask(g, B, N, counts):
    m = torch.zeros(B, N)
    for b, c in enumerate(counts):
        m[b, torch.randperm(N, generator=g)[:c]] = 1.0
    return m


def random_case(name, seed, B, N, counts, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    pred, gold = _clouds(g, B, N)
    counts = [counts] * B if isinstance(counts, int) else counts
    return _case(name, pred * scale + offset, gold * scale + offset, _random_mask(g, B, N, counts))


def tail_only_case(seed):
    """masked rows only in the last, partial 64-chunk of N = 200 (indices >= 192)"""
    g = torch.Generator().manual_seed(seed)
    pred, gold = _clouds(g, 2, 200)
    m = torch.zeros(2, 200)
    m[0, 192:] = 1.0
    m[1, [193, 194, 196, 198, 199]] = 1.0
    return _case("tail_only", pred, gold, m)


def one_row_case(seed):
    g = torch.Generator().manual_seed(seed)
    pred, gold = _clouds(g, 2, 256)
    m = torch.zeros(2, 256)
    m[0, int(torch.randint(0, 255, (1,), generator=g))] = 1.0
    m[1, 255] = 1.0
    return _case("one_row", pred, gold, m)


def wide_case(seed):
    """Clouds 16 units wide.  The 40 masked points are the slab of lowest x of gold, and the prediction of those points is far off
    (mirrored through the origin), so most masked rows are more than 10 units from every masked column and the +100 penalty loses:
    an UNMASKED column is the nearest."""
    g = torch.Generator().manual_seed(seed)
    B, N = 2, 200
    pred, gold = _clouds(g, B, N)
    m = torch.zeros(B, N)
    for b in range(B):
        idx = torch.argsort(gold[b, 0])[:40]
        m[b, idx] = 1.0
        pred[b, idx] = -gold[b][:, idx].t() + 0.05 * torch.randn(40, 3, generator=g)
    return _case("wide", pred * 8, gold * 8, m)


def ties_case(seed, duplicates=True):
    """N = 96: points 48..95 of BOTH clouds are copies of points 0..47, and the mask holds 12 of the first 48 with their copies, so
    every masked row has an exact tie between columns j and j + 48 and every masked row exists twice.  duplicates=False: the first
    half alone (N = 48, 12 masked rows)."""
    g = torch.Generator().manual_seed(seed)
    pred, gold = _clouds(g, 2, 48)
    m = _random_mask(g, 2, 48, [12, 12])
    if not duplicates:
        return _case("ties_half", pred, gold, m)
    return _case("ties", torch.cat((pred, pred), 1), torch.cat((gold, gold), 2), torch.cat((m, m), 1), ties=True)


# (seed chosen so that tests/test_loss_restatement_cpu.py's input conditions hold; see there)
def chamfer_cases():
    return [
        random_case("tiny_1x1", 1, 1, 1, 1),
        random_case("tiny_3x2", 2, 3, 2, 1),
        random_case("wave_63", 3, 2, 63, 8),
        random_case("wave_64", 4, 2, 64, 9),
        random_case("wave_65", 5, 2, 65, 17),
        random_case("wave_127_all", 6, 3, 127, 127),
        tail_only_case(7),
        one_row_case(8),
        random_case("uneven", 9, 3, 200, [1, 40, 200]),
        wide_case(22),
        random_case("off_centre", 40, 2, 200, 40, offset=50.0),
        ties_case(12),
    ]


LARGE_FUSED_N, LARGE_DIR_N = (1638, 1639, 3840), (2730, 2731, 6400)


def large_case(N):
    return random_case("large_%d" % N, 13 + N, 1, N, 40)


def nonfinite_base(seed=14):
    """B = 2, N = 70, 12 masked rows; the prediction sits 4 units off the gold cloud in every coordinate, so that multiplying a cloud by
    3e19 makes every coordinate difference at least 6e19 and every squared distance overflow fp32."""
    g = torch.Generator().manual_seed(seed)
    pred, gold = _clouds(g, 2, 70)
    return _case("nonfinite_base", pred + 4.0, gold, _random_mask(g, 2, 70, [12, 12]))


def nonfinite_cases():
    """-> (the finite base case, [(tag, case, rows_cloud)]): cloud 0 finite, cloud 1 spoilt; rows_cloud names which cloud holds the spoilt ROWS, for the
    one-direction form ("pred": chamfer_distance(pred, gold^T), "gold": the converse)"""
    out = []
    base = nonfinite_base()
    row = int(torch.nonzero(base.mask[1, 0]).reshape(-1)[3])
    a = nonfinite_base()
    a.pred[1, row, 1] = float("nan")
    out.append(("nan_in_pred", a, "pred"))
    b = nonfinite_base()
    b.gold[1, 2, row] = float("inf")
    out.append(("inf_in_gold", b, "gold"))
    c = nonfinite_base()
    c.pred[1] *= 3e19
    c.gold[1] *= 3e19
    out.append(("overflow", c, "pred"))
    return base, out


# --------------------------------------------------------------------------------------------- normal loss
NORMAL_P = (1, 255, 256, 257, 65537)
WEIGHT_KINDS = ("none", "26m+1", "01", "zero")


def make_weight(kind, P, g):
    if kind == "none":
        return None
    if kind == "zero":
        return torch.zeros(P)
    m = (torch.rand(P, generator=g) < 0.1).float()
    if P >= 2:
        m[0], m[P - 1] = 1.0, 0.0
    else:
        m[0] = 1.0
    return m * 26 + 1 if kind == "26m+1" else m


def normal_case(seed, P, kind, scale):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(1, P, 3, generator=g) * scale
    gt = torch.randn(1, P, 3, generator=g)
    return pred, gt, make_weight(kind, P, g)


def normal_reference(pred, gt, w, dtype=torch.float64):
    p = _leaf(pred, dtype)
    loss = ref_cpu.normal_prediction_loss(p, gt.to(dtype), None if w is None else w.to(dtype).view(p.shape[0], p.shape[1]))
    loss.backward()
    return dict(loss=loss.detach(), d_pred=p.grad)


# --------------------------------------------------------------------------------------------- cardinality tail and density loss
TAIL_SHAPES = ((1, 1), (1, 16), (257, 5), (257, 16), (300, 64))


def fc2w(nc):
    return torch.arange(nc, dtype=torch.float32) * 2.0            # the frozen expectation layer of the model


def tail_seed(P, nc):
    """(1, 16): a seed whose single row has its two largest logits one unit apart at scale 60.  Where one class leads by more than
    about 88 every other probability underflows fp32, and the exact gradient of that lone row, some 1e-40, is below what fp32 can
    hold: the reference's own fp32 result is then 0 and no relative distance means anything.  With more rows max|b| is set by the
    rows that have a runner-up.)"""
    return 50 if (P, nc) == (1, 16) else 30 + nc


def tail_case(seed, P, nc, scale):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(P, nc, generator=g) * scale, torch.randn(P, nc, generator=g), torch.randn(P, generator=g)


def tail_reference(logits, Rp, Rd, dtype=torch.float64):
    """-> pvec, dens, and d_logits of (pvec * Rp).sum(), of (dens * Rd).sum() and of their sum"""
    lg = _leaf(logits, dtype)
    p = torch.softmax(lg, dim=1)
    d = (p * fc2w(lg.shape[1]).to(dtype)).sum(1)
    lp, ld = (p * Rp.to(dtype)).sum(), (d * Rd.to(dtype)).sum()
    gp, = torch.autograd.grad(lp, lg, retain_graph=True)
    gd, = torch.autograd.grad(ld, lg, retain_graph=True)
    gb, = torch.autograd.grad(lp + ld, lg)
    return dict(pvec=p.detach(), dens=d.detach(), d_from_pvec=gp, d_from_dens=gd, d_from_both=gb)


def soft_labels(P, nc, g, pergroup=2):
    """MLSP/mlsp.py:259-263: the count's two neighbouring classes share the label; -> (target_vec [P,nc], target [P])"""
    count = torch.randint(0, max(1, pergroup * (nc - 1) + 1), (P,), generator=g).double()
    c1, c2 = torch.floor(count / pergroup).long(), torch.ceil(count / pergroup).long()
    eye = torch.eye(nc, dtype=torch.float64)
    return ((eye[c1] + eye[c2]) / 2).float(), count.float()


def density_case(seed, P, nc, kind):
    """hand-made p_vec rows (positive, summing to 1 for nc > 1), densities near the targets, some equal to them"""
    g = torch.Generator().manual_seed(seed)
    pvec = torch.rand(P, nc, generator=g) + 0.05
    pvec = pvec / pvec.sum(1, keepdim=True) if nc > 1 else pvec / 1.5      # nc = 1: see test_gpu_losses.test_density_loss
    tvec, target = soft_labels(P, nc, g)
    dens = target + torch.randn(P, generator=g)
    dens[::3] = target[::3]
    return pvec, dens, tvec, target, make_weight(kind, P, g)


def density_zero_case(seed, P=257, nc=16):
    """p_vec with exact zeros, under a label and elsewhere: reaches the + 1e-10"""
    pvec, dens, tvec, target, _ = density_case(seed, P, nc, "none")
    pvec[::2, ::2] = 0.0
    return pvec, dens, tvec, target, None


def density_reference(pvec, dens, tvec, target, m, dtype=torch.float64, dweight=1.0):
    """-> kl, mae and (d_pvec, d_dens) of kl, of mae and of kl + mae"""
    p, d = _leaf(pvec, dtype), _leaf(dens, dtype)
    args = types.SimpleNamespace(Density_weight=dweight)
    kl, mae = ref_cpu.densityloss(args, {"density": p, "density_mse": d}, target.to(dtype), tvec.to(dtype),
                                  None if m is None else m.to(dtype))
    out = dict(kl=kl.detach(), mae=mae.detach())
    for tag, l in (("kl", kl), ("mae", mae), ("both", kl + mae)):
        gp, gd = torch.autograd.grad(l, (p, d), retain_graph=True, allow_unused=True)
        out["d_pvec_" + tag] = gp if gp is not None else torch.zeros_like(p)
        out["d_dens_" + tag] = gd if gd is not None else torch.zeros_like(d)
    return out


def tail_density_reference(logits, tvec, target, m, dtype=torch.float64):
    """density_tail feeding densityloss: -> kl, mae, d_logits of kl + mae"""
    lg = _leaf(logits, dtype)
    p = torch.softmax(lg, dim=1)
    d = (p * fc2w(lg.shape[1]).to(dtype)).sum(1)
    args = types.SimpleNamespace(Density_weight=1.0)
    kl, mae = ref_cpu.densityloss(args, {"density": p, "density_mse": d}, target.to(dtype), tvec.to(dtype),
                                  None if m is None else m.to(dtype))
    (kl + mae).backward()
    return dict(kl=kl.detach(), mae=mae.detach(), d_logits=lg.grad)
