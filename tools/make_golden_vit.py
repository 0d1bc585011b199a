"""Generate tests/golden/vitblock_*.npz and vitenc_*.npz: the UNMODIFIED reference's Point-BERT transformer stack (PointDA/model_utils.py:
Block, TransformerEncoder), run on the CPU in fp32 with autograd.  Build-container only (imports the reference through
tools/ref_import.py); the fixtures are numeric and string arrays.

    python tools/make_golden_vit.py

ref_import's DropPath stub cannot be constructed, so the reference runs with drop_path = 0, where it uses nn.Identity.  The LayerNorm
weights and biases are moved off their (1, 0) defaults (seeded) so that they matter.

Every case stores x (and pos for the encoder), every parameter (key "p.<state_dict key>"), the state_dict key order ("keys"), out (and
"feat0", the one entry of feature_list), a fixed random R (and R2 for feat0), and the gradients of (out * R).sum() [+ (feat0 * R2).sum()]
with respect to the inputs ("g.x", "g.pos") and every parameter ("g.<state_dict key>"); "dims" = [B, L, dim, heads, depth].
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def npy(t):
    return t.detach().cpu().numpy()


def perturb_norms(mod, g):
    with torch.no_grad():
        for m in mod.modules():
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.add_(0.2 * torch.randn(m.weight.shape, generator=g))
                m.bias.add_(0.1 * torch.randn(m.bias.shape, generator=g))


def params_of(mod, c):
    c["keys"] = np.array(list(mod.state_dict().keys()))
    for name, p in mod.named_parameters():
        c["p." + name], c["g." + name] = npy(p), npy(p.grad)
    return c


def block_case(seed, B, L, dim, heads):
    from PointDA.model_utils import Block
    torch.manual_seed(seed)
    blk = Block(dim, heads, qkv_bias=False)
    g = torch.Generator().manual_seed(1000 + seed)
    perturb_norms(blk, g)
    x = torch.randn(B, L, dim, generator=g).requires_grad_(True)
    out = blk(x)
    R = torch.randn(out.shape, generator=g)
    (out * R).sum().backward()
    return params_of(blk, {"x": npy(x), "out": npy(out), "R": npy(R), "g.x": npy(x.grad), "dims": np.array([B, L, dim, heads, 1])})


def encoder_case(seed, B, L, dim, heads, depth):
    from PointDA.model_utils import TransformerEncoder
    torch.manual_seed(seed)
    enc = TransformerEncoder(embed_dim=dim, depth=depth, num_heads=heads, qkv_bias=True)
    g = torch.Generator().manual_seed(1000 + seed)
    perturb_norms(enc, g)
    x = torch.randn(B, L, dim, generator=g).requires_grad_(True)
    pos = (0.5 * torch.randn(B, L, dim, generator=g)).requires_grad_(True)
    out, feats = enc(x, pos)
    assert len(feats) == 1
    R, R2 = torch.randn(out.shape, generator=g), torch.randn(out.shape, generator=g)
    ((out * R).sum() + (feats[0] * R2).sum()).backward()
    return params_of(enc, {"x": npy(x), "pos": npy(pos), "out": npy(out), "feat0": npy(feats[0]), "R": npy(R), "R2": npy(R2),
                           "g.x": npy(x.grad), "g.pos": npy(pos.grad), "dims": np.array([B, L, dim, heads, depth])})


def main():
    ref_import.install_stubs()
    for p in (ref_import.REF_ROOT + "/PointDA", ref_import.REF_ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(8)
    for name, c in (("vitblock_s0_B2_L65_d48_h6.npz", block_case(0, 2, 65, 48, 6)),
                    ("vitenc_s1_B2_L9_d32_h4_depth4.npz", encoder_case(1, 2, 9, 32, 4, 4))):
        np.savez_compressed(os.path.join(OUT, name), **c)
        print(name, os.path.getsize(os.path.join(OUT, name)), list(c["keys"])[:4])


if __name__ == "__main__":
    main()
