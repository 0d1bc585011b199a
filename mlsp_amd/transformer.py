"""The vector-attention block of the Hengshuang Point Transformer on MI355X.

Mirrors PointDA/hengshuang_transformer/transformer.py: same class name, constructor arguments, tensor layouts ([B,N,3] coordinates,
[B,N,d_points] features) and state_dict keys (`fc1.*`, `fc2.*`, `fc_delta.{0,2}.*`, `fc_gamma.{0,2}.*`, `w_qs.weight`, `w_ks.weight`,
`w_vs.weight`): the nn.Linear / nn.Sequential members hold the parameters only, the arithmetic is functional.vector_attention
(csrc/vecattn.hip) between pointmlp GEMMs.  No CPU fallback.

The models around the block (TransitionDown / TransitionUp / Backbone / PointTransformerCls, Seg, Def) are mlsp_amd/hengshuang_model.py.
Not built: gradients with respect to the coordinates, and a gradient through the returned attention weights.
"""
import torch
import torch.nn as nn

from . import _lib
from . import functional as Fh
from .pointnet2 import knn_point


class TransformerBlock(nn.Module):
    def __init__(self, d_points, d_model, k) -> None:
        super().__init__()
        self.fc1 = nn.Linear(d_points, d_model)
        self.fc2 = nn.Linear(d_model, d_points)
        self.fc_delta = nn.Sequential(nn.Linear(3, d_model), nn.ReLU(), nn.Linear(d_model, d_model))
        self.fc_gamma = nn.Sequential(nn.Linear(d_model, d_model), nn.ReLU(), nn.Linear(d_model, d_model))
        self.w_qs = nn.Linear(d_model, d_model, bias=False)
        self.w_ks = nn.Linear(d_model, d_model, bias=False)
        self.w_vs = nn.Linear(d_model, d_model, bias=False)
        self.k = k

    def neighbours(self, xyz):
        """transformer.py:29-30: the min(k, N) nearest points of every point among its own cloud, nearest first (itself first) -> int64
        [B,N,min(k,N)]"""
        return knn_point(min(self.k, xyz.shape[1]), xyz, xyz)

    def forward(self, xyz, features, knn_idx=None):
        """xyz [B,N,3], features [B,N,d_points] -> (out [B,N,d_points], attn [B,N,k_eff,d_model]), k_eff = min(k, N).  `knn_idx` (int64
        [B,N,k_eff], entries in [0, N)) pins the neighbour graph instead of searching it.  attn carries no gradient."""
        _lib.load()
        _lib.require_gpu(xyz, features)
        assert xyz.dim() == 3 and xyz.shape[-1] == 3 and features.dim() == 3 and features.shape[:2] == xyz.shape[:2], (xyz.shape, features.shape)
        B, N, _ = xyz.shape
        if knn_idx is None:
            knn_idx = self.neighbours(xyz)
        else:
            _lib.require_gpu(knn_idx)
            if knn_idx.dim() != 3 or knn_idx.shape[:2] != (B, N) or int(knn_idx.min()) < 0 or int(knn_idx.max()) >= N:
                raise ValueError("knn_idx: expected [B, N, k] indices in [0, N), got shape %s" % (tuple(knn_idx.shape),))
        idx32 = knn_idx.to(torch.int32).contiguous()
        k_eff = idx32.shape[2]
        d = self.fc1.out_features
        f = features.reshape(B * N, -1).float()
        x = Fh.pointmlp(f, self.fc1.weight, bias=self.fc1.bias)
        q, kk, v = (Fh.pointmlp(x, w.weight) for w in (self.w_qs, self.w_ks, self.w_vs))
        res, attn = Fh.vector_attention(xyz.detach().reshape(B * N, 3).float(), idx32, q, kk, v,
                                        self.fc_delta[0].weight, self.fc_delta[0].bias, self.fc_delta[2].weight, self.fc_delta[2].bias,
                                        self.fc_gamma[0].weight, self.fc_gamma[0].bias, self.fc_gamma[2].weight, self.fc_gamma[2].bias)
        out = Fh.pointmlp(res, self.fc2.weight, bias=self.fc2.bias) + f
        return out.view(B, N, -1), attn.view(B, N, k_eff, d)
