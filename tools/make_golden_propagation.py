"""Generate tests/golden/dgprop_*.npz: the UNMODIFIED reference's DGCNN_Propagation (PointDA/Models.py:289-363), run on the CPU in fp32
with autograd.  Build-container only (imports the reference through tools/ref_import.py); the fixtures are numeric and string arrays.

    python tools/make_golden_propagation.py

knn_cuda is not installed anywhere: after install_stubs() its KNN is a small plain-torch class defined here (squared distances, a stable
ascending sort, the first k; it honours transpose_mode).

  dgprop_s0_B2_G8_N16_k4_c16_m32.npz   the reference's class and forward with its two Sequentials replaced by narrower ones of the same three
                                       layers (in 16, mid 32); every parameter and gradient stored ("p.<key>", "g.<key>"); GroupNorm weights
                                       drawn from N(0,1) (some negative), biases non-zero
  dgprop_s1_B2_G8_N16_k4_ref.npz       the reference's own widths; the conv weights (3 MB) are not stored: tests/dgprop_restatement.hash_fill
                                       makes them from their flat index and the seeds in "wseed" (scale in "wscale"); stored: the GroupNorm
                                       parameters and their gradients, every 16th row of each conv weight gradient ("g16.<key>")
Both store coor, f, coor_q, f_q, out, a fixed random R, the gradients of (out * R).sum() with respect to f and f_q ("g.f", "g.f_q"), the
stage graphs idx1, idx2 and dims = [B, G, N, k, in_dim, mid_dim].

The seed is re-drawn until (a) in every query's neighbour list of both graphs consecutive squared distances up to the (k+1)-th differ by
more than 1e-4 of the larger, and (b) no output entry's best and second-best slot (of either stage) are closer than 1e-4 of that stage's
largest output magnitude -- then neither a neighbour set nor a selection depends on rounding.  (b) is attainable for the narrow case.  At
the reference's widths it is not: 2 x 16 x (512 + 384) entries whose top-two gap has a density of order 10 per unit of the largest
magnitude leave some thirty entries under 1e-4 in every draw.  There the tool takes, of MAX_DRAWS draws that satisfy (a), the one with the
widest margin and stores it ("sel_margin"); the tests route gradients through recorded selections and do not rely on it.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_import  # noqa: E402
import dgprop_restatement as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
MARGIN = 1e-4
MAX_DRAWS = 300


class KNN:
    """knn_cuda.KNN in plain torch: ref / query [B,C,N] (transpose_mode False) or [B,N,C] (True) -> (dist, idx) [B,k,Nq] / [B,Nq,k]"""

    def __init__(self, k=1, transpose_mode=False):
        self.k, self.transpose_mode = k, transpose_mode

    def __call__(self, ref, query):
        if not self.transpose_mode:
            ref, query = ref.transpose(1, 2), query.transpose(1, 2)
        d2 = ((query.unsqueeze(2) - ref.unsqueeze(1)) ** 2).sum(-1)
        d, idx = d2.sort(dim=-1, stable=True)
        d, idx = d[:, :, :self.k], idx[:, :, :self.k]
        if not self.transpose_mode:
            d, idx = d.transpose(1, 2).contiguous(), idx.transpose(1, 2).contiguous()
        return d.sqrt(), idx

    forward = __call__


def npy(t):
    return t.detach().cpu().numpy()


def graphs_separated(k, coor, coor_q):
    for ref in (coor, coor_q):
        d = R.knn(k, ref.transpose(1, 2).double(), coor_q.transpose(1, 2).double())[1].sort(dim=-1)[0][:, :, :k + 1]
        if not bool(((d[:, :, 1:] - d[:, :, :-1]) > MARGIN * d[:, :, 1:]).all()):
            return False
    return True


def selection_margin(params, coor, f, coor_q, f_q, idx1, idx2):
    worst = float("inf")
    for z in R.forward(params, coor, f, coor_q, f_q, idx1, idx2, dtype=torch.float64, return_edges=True):
        top = z.topk(2, dim=-1)[0] if z.shape[-1] > 1 else None
        if top is not None:
            worst = min(worst, float(((top[..., 0] - top[..., 1]).min() / z.abs().max())))
    return worst


def draw(seed, B, G, N, k, in_dim, mid_dim, ref_width):
    from PointDA.Models import DGCNN_Propagation
    torch.manual_seed(seed)
    m = DGCNN_Propagation(k=k)
    g = torch.Generator().manual_seed(1000 + seed)
    c = {}
    if ref_width:
        assert (in_dim, mid_dim) == (384, 512)
        seeds, scales = [2 * seed + 11, 2 * seed + 12], [float(np.sqrt(3.0 / (2 * in_dim))), float(np.sqrt(3.0 / (2 * mid_dim)))]
        with torch.no_grad():
            for layer, s, sc in zip((m.layer1, m.layer2), seeds, scales):
                layer[0].weight.copy_(torch.from_numpy(R.hash_fill(tuple(layer[0].weight.shape), s, sc)))
        c["wseed"], c["wscale"] = np.array(seeds), np.array(scales, dtype=np.float64)
    else:
        nn = torch.nn
        m.layer1 = nn.Sequential(nn.Conv2d(2 * in_dim, mid_dim, kernel_size=1, bias=False), nn.GroupNorm(4, mid_dim), nn.LeakyReLU(negative_slope=0.2))
        m.layer2 = nn.Sequential(nn.Conv2d(2 * mid_dim, in_dim, kernel_size=1, bias=False), nn.GroupNorm(4, in_dim), nn.LeakyReLU(negative_slope=0.2))
    with torch.no_grad():
        for layer in (m.layer1, m.layer2):
            layer[1].weight.copy_(torch.randn(layer[1].weight.shape, generator=g))
            layer[1].bias.copy_(0.3 * torch.randn(layer[1].bias.shape, generator=g))
    coor, coor_q = torch.randn(B, 3, G, generator=g), torch.randn(B, 3, N, generator=g)
    f = torch.randn(B, in_dim, G, generator=g).requires_grad_(True)
    f_q = torch.randn(B, in_dim, N, generator=g).requires_grad_(True)
    if not graphs_separated(k, coor, coor_q):
        return None, None
    idx1 = R.knn(k, coor.transpose(1, 2), coor_q.transpose(1, 2))[0]
    idx2 = R.knn(k, coor_q.transpose(1, 2), coor_q.transpose(1, 2))[0]
    params = {key: v.detach() for key, v in m.state_dict().items()}
    margin = selection_margin(params, coor, f.detach(), coor_q, f_q.detach(), idx1, idx2)

    def finish():
        out = m(coor, f, coor_q, f_q)
        Rw = torch.randn(out.shape, generator=g)
        (out * Rw).sum().backward()
        c.update({"coor": npy(coor), "f": npy(f), "coor_q": npy(coor_q), "f_q": npy(f_q), "out": npy(out), "R": npy(Rw), "g.f": npy(f.grad),
                  "g.f_q": npy(f_q.grad), "idx1": npy(idx1).astype(np.int32), "idx2": npy(idx2).astype(np.int32),
                  "dims": np.array([B, G, N, k, in_dim, mid_dim]), "keys": np.array(list(m.state_dict().keys())), "seed": np.array(seed),
                  "sel_margin": np.array(margin)})
        for name, p in m.named_parameters():
            if ref_width and p.dim() == 4:
                c["g16." + name] = npy(p.grad)[::16]
            else:
                c["p." + name], c["g." + name] = npy(p), npy(p.grad)
        return c
    return margin, finish


def case(first_seed, B, G, N, k, in_dim, mid_dim, ref_width):
    best = (-1.0, None)
    for i in range(MAX_DRAWS):
        margin, finish = draw(first_seed + 100 * i, B, G, N, k, in_dim, mid_dim, ref_width)
        if margin is None:
            continue
        if margin > best[0]:
            best = (margin, finish)
        if margin > MARGIN:
            break
    assert best[1] is not None
    assert ref_width or best[0] > MARGIN, best[0]
    return best[1]()


def main():
    ref_import.install_stubs()
    sys.modules["knn_cuda"].KNN = KNN
    for p in (ref_import.REF_ROOT + "/PointDA", ref_import.REF_ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(8)
    for name, c in (("dgprop_s0_B2_G8_N16_k4_c16_m32.npz", case(0, 2, 8, 16, 4, 16, 32, False)),
                    ("dgprop_s1_B2_G8_N16_k4_ref.npz", case(1, 2, 8, 16, 4, 384, 512, True))):
        np.savez_compressed(os.path.join(OUT, name), **c)
        size = os.path.getsize(os.path.join(OUT, name))
        print(name, size, "seed", int(c["seed"]), "selection margin %.2e" % float(c["sel_margin"]))
        assert size < 1000000, size


if __name__ == "__main__":
    main()
