"""The Point-BERT-style transformer encoder of the reference (PointDA/model_utils.py:201-289: Mlp, Attention, Block, TransformerEncoder)
on MI355X.

Same class names, constructor arguments and defaults, tensor layouts ([B,L,C]) and state_dict keys, registration order included (`norm1`,
`norm2`, `mlp.fc1`, `mlp.fc2`, `attn.qkv`, `attn.proj`): the nn.Linear / nn.LayerNorm members hold the parameters only.  The arithmetic is
pointmlp GEMMs with functional.layernorm / mhsa / gelu (csrc/attn.hip) between them; a block is

    u1, y1 = layernorm(x [+ pos])            norm1, the encoder's `x + pos` folded in
    qkv    = pointmlp(y1, attn.qkv)
    o      = mhsa(qkv)                       one launch, nothing of size L^2 in memory
    p      = pointmlp(o, attn.proj)
    u2, y2 = layernorm(u1 + s1 * p)          the residual add, DropPath's scale s1 and norm2 in one pass
    h      = gelu(pointmlp(y2, mlp.fc1))
    m      = pointmlp(h, mlp.fc2)
    out    = u2 + s2 * m                     layernorm(..., weight=None)

No CPU fallback.  `drop` / `attn_drop` > 0 (which the reference's encoder never sets) raise NotImplementedError at construction.

The model around the stack -- PointTransformer, Group, Encoder -- is mlsp_amd/pointbert.py (DGCNN_Propagation: mlsp_amd/propagation.py).
"""
import torch
import torch.nn as nn

from . import _lib
from . import functional as Fh

_forced_masks = None       # test hook: keep masks consumed by successive DropPath draws (forced_drop_masks)


class forced_drop_masks:
    """Context manager (tests only), in the style of functional.forced_selections: successive DropPath draws of a training forward take
    these [B] keep masks (1 keep, 0 drop), in call order (two per Block: after the attention, after the MLP), instead of drawing them."""

    def __init__(self, masks):
        self.masks = list(masks)

    def __enter__(self):
        global _forced_masks
        _forced_masks = list(self.masks)
        return self

    def __exit__(self, *exc):
        global _forced_masks
        _forced_masks = None
        return False


class DropPath(nn.Module):
    """Stochastic depth per sample (timm's DropPath, scale_by_keep): the identity in eval mode and at rate 0; in training a sample's branch is
    kept with probability 1 - drop_prob and scaled by 1 / (1 - drop_prob).  The module does no arithmetic on the branch: sample_scale()
    hands mask / keep_prob to functional.layernorm, which applies it inside the residual add."""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def sample_scale(self, B, device):
        """-> [B] float32 on `device`, or None where the module is the identity"""
        if not self.training or self.drop_prob == 0.0:
            return None
        keep = 1.0 - self.drop_prob
        if _forced_masks is not None:
            mask = _forced_masks.pop(0).to(device=device, dtype=torch.float32)
            assert mask.shape == (B,), (mask.shape, B)
        else:
            mask = torch.empty((B,), dtype=torch.float32, device=device).bernoulli_(keep)
        return mask / keep if keep > 0.0 else mask

    def forward(self, x):
        s = self.sample_scale(x.shape[0], x.device)
        if s is None:
            return x
        _lib.require_gpu(x)
        rows = x.reshape(x.shape[0], -1).float()       # 0 + s * x through the residual-add kernel: one sample per row
        return Fh.layernorm(torch.zeros_like(rows), None, None, 0.0, add=rows, sample_scale=s, rows_per_sample=1)[0].view_as(x)

    def extra_repr(self):
        return "drop_prob=%g" % self.drop_prob


def _no_dropout(**rates):
    for name, p in rates.items():
        if p > 0:
            raise NotImplementedError("%s=%g: dropout inside the transformer encoder is not built (the reference's encoder never sets it)"
                                      % (name, p))


def _gelu_only(act_layer):
    if act_layer is not nn.GELU:
        raise NotImplementedError("act_layer=%r: only nn.GELU (the erf form) has a kernel" % (act_layer,))


def _rows_of(x):
    """[B,L,C] -> (B, L, [B*L, C] float32 rows)"""
    _lib.load()
    _lib.require_gpu(x)
    assert x.dim() == 3, x.shape
    B, L, C = x.shape
    return B, L, x.reshape(B * L, C).float()


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        _no_dropout(drop=drop)
        _gelu_only(act_layer)
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features, out_features)
        self.drop = nn.Dropout(drop)

    def rows(self, y):
        h = Fh.gelu(Fh.pointmlp(y, self.fc1.weight, bias=self.fc1.bias))
        return Fh.pointmlp(h, self.fc2.weight, bias=self.fc2.bias)

    def forward(self, x):
        B, L, y = _rows_of(x)
        return self.rows(y).view(B, L, -1)


class Attention(nn.Module):
    def __init__(self, dim, num_heads=8, qkv_bias=False, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        _no_dropout(attn_drop=attn_drop, proj_drop=proj_drop)
        assert dim % num_heads == 0, (dim, num_heads)
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)

    def rows(self, y, B, L):
        qkv = Fh.pointmlp(y, self.qkv.weight, bias=self.qkv.bias)
        o, _ = Fh.mhsa(qkv, B, L, self.num_heads, self.scale)
        return Fh.pointmlp(o, self.proj.weight, bias=self.proj.bias)

    def forward(self, x):
        B, L, y = _rows_of(x)
        return self.rows(y, B, L).view(B, L, -1)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm):
        super().__init__()
        if norm_layer is not nn.LayerNorm:
            raise NotImplementedError("norm_layer=%r: only nn.LayerNorm has a kernel" % (norm_layer,))
        self.norm1 = norm_layer(dim)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        mlp_hidden_dim = int(dim * mlp_ratio)
        self.mlp = Mlp(in_features=dim, hidden_features=mlp_hidden_dim, act_layer=act_layer, drop=drop)
        self.attn = Attention(dim, num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale, attn_drop=attn_drop, proj_drop=drop)

    def _scale(self, B, device):
        return self.drop_path.sample_scale(B, device) if isinstance(self.drop_path, DropPath) else None

    def rows(self, x, B, L, add=None):
        """x [B*L, C] (+ add [B*L, C]: the encoder's position embedding) -> [B*L, C]"""
        n1, n2 = self.norm1, self.norm2
        u1, y1, _, _ = Fh.layernorm(x, n1.weight, n1.bias, n1.eps, add=add)
        p = self.attn.rows(y1, B, L)
        u2, y2, _, _ = Fh.layernorm(u1, n2.weight, n2.bias, n2.eps, add=p, sample_scale=self._scale(B, x.device), rows_per_sample=L)
        m = self.mlp.rows(y2)
        return Fh.layernorm(u2, None, None, 0.0, add=m, sample_scale=self._scale(B, x.device), rows_per_sample=L)[0]

    def forward(self, x):
        B, L, r = _rows_of(x)
        return self.rows(r, B, L).view(B, L, -1)


class TransformerEncoder(nn.Module):
    """ Transformer Encoder without hierarchical structure
    """
    def __init__(self, embed_dim=768, depth=4, num_heads=12, mlp_ratio=4., qkv_bias=False, qk_scale=None,
                 drop_rate=0., attn_drop_rate=0., drop_path_rate=0.):
        super().__init__()
        self.blocks = nn.ModuleList([
            Block(dim=embed_dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale,
                  drop=drop_rate, attn_drop=attn_drop_rate,
                  drop_path=drop_path_rate[i] if isinstance(drop_path_rate, list) else drop_path_rate)
            for i in range(depth)])

    def forward(self, x, pos):
        B, L, r = _rows_of(x)
        _, _, p = _rows_of(pos)
        assert p.shape == r.shape, (pos.shape, x.shape)
        feature_list = []
        fetch_idx = [3, 7, 11]
        for i, block in enumerate(self.blocks):
            r = block.rows(r, B, L, add=p)
            if i in fetch_idx:
                feature_list.append(r.view(B, L, -1))
        return r.view(B, L, -1), feature_list
