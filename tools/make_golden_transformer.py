"""Generate tests/golden/tblock_*.npz: the UNMODIFIED reference's vector-attention block
(PointDA/hengshuang_transformer/transformer.py: TransformerBlock), run on the CPU in fp32 with autograd.  Build-container only (imports
the reference through tools/ref_import.py); the fixtures are numeric arrays.

    python tools/make_golden_transformer.py

Every case stores xyz ~ U[-1,1)^3, the features, every parameter (key "p.<state_dict key>"), the reference's knn_idx
(square_distance(xyz, xyz).argsort()[:, :, :k], as its forward computes it), out, attn, a fixed random R and the gradients of
(out * R).sum() with respect to the features ("g.features") and every parameter ("g.<state_dict key>").
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


def case(seed, B, N, k, d_points, d_model):
    from PointDA.hengshuang_transformer.transformer import TransformerBlock
    from PointDA.hengshuang_transformer.pointnet_util import square_distance
    torch.manual_seed(seed)
    blk = TransformerBlock(d_points, d_model, k)
    g = torch.Generator().manual_seed(1000 + seed)
    xyz = torch.rand(B, N, 3, generator=g) * 2 - 1
    feat = torch.randn(B, N, d_points, generator=g).requires_grad_(True)
    out, attn = blk(xyz, feat)
    R = torch.randn(out.shape, generator=g)
    (out * R).sum().backward()
    c = {"xyz": npy(xyz), "features": npy(feat), "knn_idx": npy(square_distance(xyz, xyz).argsort()[:, :, :k]),
         "out": npy(out), "attn": npy(attn), "R": npy(R), "g.features": npy(feat.grad),
         "dims": np.array([B, N, k, d_points, d_model])}
    for name, p in blk.named_parameters():
        c["p." + name], c["g." + name] = npy(p), npy(p.grad)
    return c


def main():
    ref_import.install_stubs()
    for p in (ref_import.REF_ROOT + "/PointDA", ref_import.REF_ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)
    torch.set_num_threads(8)
    for name, args in (("tblock_s0_B2_N64_k16.npz", (0, 2, 64, 16, 32, 64)), ("tblock_s1_B2_N8_k16.npz", (1, 2, 8, 16, 64, 32))):
        c = case(*args)
        np.savez_compressed(os.path.join(OUT, name), **c)
        print(name, os.path.getsize(os.path.join(OUT, name)), "attn", c["attn"].shape)


if __name__ == "__main__":
    main()
