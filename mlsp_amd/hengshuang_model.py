"""The Point Transformer models of the reference (PointDA/hengshuang_transformer/hengshuang_model.py) around the vector-attention block,
on MI355X.

Same class names, constructor arguments, `cfg` attribute reads (the reference's mix of `cfg.nblocks` and `cfg.model.nblocks` included),
tensor layouts, return values and state_dict keys in the reference's order (the parameterless SwapAxes slots of TransitionUp.fc1 / fc2
keep `fc1.0.*` and `fc1.2.*` where they are).  The nn.Linear / nn.BatchNorm1d members hold the parameters only; the arithmetic, on row
matrices:

    Linear + ReLU stacks   identity-BatchNorm eval-mode pointmlp (seg_models._linear_act), the last layer a plain pointmlp
    TransformerBlock       transformer.TransformerBlock (csrc/vecattn.hip); the kNN of a level is searched once and serves the
                           backbone's block and the decoder's block of that level (the reference searches it twice, same result)
    TransitionDown         PointNetSetAbstraction(k, 0, nneighbor, channels[0], channels[1:], group_all=False, knn=True), unchanged
    TransitionUp           Linear + BatchNorm1d + ReLU twice: pointmlp with batch statistics over all B N rows (what the two axis swaps
                           amount to); then functional.interp3_add (csrc/pyramid.hip): feats2 + the 3-NN interpolation of feats1 in one
                           pass, no interpolated tensor and no torch add
    points.mean(1)         functional.cloud_mean (csrc/pyramid.hip)
    DefRec                 RegionReconstruction.rows(point rows [B N, 32], global feature [B, 512]): the global half of conv1 enters as a
                           per-cloud bias, cat(points^T, global.repeat) [B, 544, N] is never built

Pinning the graph.  Every forward takes `graph=None`: a PyramidGraph carrying, per level, the FPS indices and the TransitionDown kNN, the
TransformerBlock kNN and the 3-NN of every TransitionUp, used instead of the searches (entries left None are searched).  Without it the
model searches for itself; the first FPS sample of level i is `backbone.transition_downs[i].sa.fps_start` ([B] tensor; None: drawn at
random as the reference does).  `with recorded_graph() as g:` collects what a forward used.

Selecting ops.  The only discrete choice besides the graph is the neighbourhood max of every TransitionDown; it goes through
functional._selection_hook, so functional.recorded_selections / forced_selections cover the models.  Call order: transition_downs[0],
[1], ... -- one [B S_i, C_i] uint8 slot tensor each (the fused last conv + max, or segmax where the shape falls back to it).

Refusals, before any launch: CPU tensors (MlspLibraryError), `nneighbor` larger than a level's point count in a TransitionDown
(ValueError), a TransitionUp fed from a level of exactly two points (ValueError, as PointNetFeaturePropagation), transformer_dim % 4 != 0
(the block's own refusal).

No CPU fallback.  Not built: gradients with respect to the coordinates and through the returned attention, dropout, bf16 storage.
"""
import contextlib

import torch
import torch.nn as nn

from . import _lib
from . import functional as Fh
from .model_utils import _bn_buffers, flushing_forward
from .pointnet2 import PointNetFeaturePropagation, PointNetSetAbstraction, _pinned, knn_point
from .seg_models import _linear_act
from .transformer import TransformerBlock


class PyramidGraph:
    """The discrete structure of one forward.  With L = nblocks + 1 levels (level 0 = the input cloud of N_0 points, N_i = npoint // 4^i):
        fps_idx[i]    int64 [B, N_{i+1}]              centres TransitionDown i samples from level i
        down_knn[i]   int64 [B, N_{i+1}, nneighbor]   their neighbourhoods in level i, nearest first
        block_knn[l]  int64 [B, N_l, min(k, N_l)]     the TransformerBlock kNN of level l (itself first)
        up_knn[i]     int64 [B, N_l, 3], l = nblocks - 1 - i: the three nearest points of level l + 1 for transition_ups[i]
                      (None where level l + 1 has one point)
    Entries that are None are searched."""

    def __init__(self, nblocks):
        self.fps_idx = [None] * nblocks
        self.down_knn = [None] * nblocks
        self.block_knn = [None] * (nblocks + 1)
        self.up_knn = [None] * nblocks


_graph_record = None     # test hook: the PyramidGraph the next forwards fill (recorded_graph)


@contextlib.contextmanager
def recorded_graph():
    """Context manager (tests, parity tools): yields a holder whose `.graph` is the PyramidGraph of the last model forward inside the block."""
    global _graph_record

    class _Holder:
        graph = None
    prev, _graph_record = _graph_record, _Holder()
    try:
        yield _graph_record
    finally:
        _graph_record = prev


def _stack(x, layers):
    """nn.Sequential(Linear, ReLU, ..., Linear) on rows: Linear + ReLU pairs fused, the last Linear plain"""
    lin = [m for m in layers if isinstance(m, nn.Linear)]
    for m in lin[:-1]:
        x = _linear_act(x, m.weight, m.bias, Fh.ACT_RELU)
    return Fh.pointmlp(x, lin[-1].weight, bias=lin[-1].bias)


def _check_down(nsample, npoint, N):
    if nsample > N or npoint > N:
        raise ValueError("TransitionDown(k=%d, nneighbor=%d) on clouds of %d points" % (npoint, nsample, N))


def _check_up(S):
    if S == 2:
        raise ValueError("TransitionUp needs at least three sampled points (or exactly one), got 2")


class TransitionDown(nn.Module):
    def __init__(self, k, nneighbor, channels):
        super().__init__()
        self.sa = PointNetSetAbstraction(k, 0, nneighbor, channels[0], channels[1:], group_all=False, knn=True)

    def forward(self, xyz, points, fps_idx=None, knn_idx=None, chosen=None):
        """xyz [B,N,3], points [B,N,channels[0]-3] -> new_xyz [B,k,3], new_points [B,k,channels[-1]].  `fps_idx` [B,k] / `knn_idx`
        [B,k,nneighbor] pin the sampling / the neighbourhoods; `chosen` (a list) receives the (fps_idx, knn_idx) used."""
        _check_down(self.sa.nsample, self.sa.npoint, xyz.shape[1])
        _lib.load()
        _lib.require_gpu(xyz, points)
        return self.sa(xyz, points, fps_idx=fps_idx, idx=knn_idx, chosen=chosen)


class SwapAxes(nn.Module):
    """x.transpose(1, 2): the parameterless slots 1 and 3 of TransitionUp.fc1 / fc2 (the rows path needs neither)"""

    def forward(self, x):
        return x.transpose(1, 2)


class TransitionUp(nn.Module):
    def __init__(self, dim1, dim2, dim_out):
        super().__init__()
        self.fc1 = nn.Sequential(
            nn.Linear(dim1, dim_out),
            SwapAxes(),
            nn.BatchNorm1d(dim_out),
            SwapAxes(),
            nn.ReLU(),
        )
        self.fc2 = nn.Sequential(
            nn.Linear(dim2, dim_out),
            SwapAxes(),
            nn.BatchNorm1d(dim_out),
            SwapAxes(),
            nn.ReLU(),
        )
        self.fp = PointNetFeaturePropagation(-1, [])

    def _branch(self, seq, rows):
        lin, bn = seq[0], seq[2]
        rm, rv = _bn_buffers(bn, self.training)
        return Fh.pointmlp(rows, lin.weight, bias=lin.bias, gamma=bn.weight, beta=bn.bias, run_mean=rm, run_var=rv, training=self.training,
                           act=Fh.ACT_RELU, momentum=bn.momentum, eps=bn.eps)

    @flushing_forward
    def forward(self, xyz1, points1, xyz2, points2, knn_idx=None, chosen=None):
        """xyz1 [B,S,3], points1 [B,S,dim1] (the coarse level), xyz2 [B,N,3], points2 [B,N,dim2] -> [B,N,dim_out].  `knn_idx` [B,N,3]
        pins the three nearest coarse points of every fine point; `chosen` (a list) receives the one used (None for S == 1)."""
        B, S, _ = xyz1.shape
        N = xyz2.shape[1]
        _check_up(S)
        _lib.load()
        _lib.require_gpu(xyz1, points1, xyz2, points2)
        feats1 = self._branch(self.fc1, points1.reshape(B * S, -1).float()).view(B, S, -1)
        feats2 = self._branch(self.fc2, points2.reshape(B * N, -1).float()).view(B, N, -1)
        idx = dist = None
        if S > 1:
            with torch.no_grad():
                if knn_idx is None:
                    idx, dist = knn_point(3, xyz1, xyz2, return_dist=True)
                else:
                    idx = _pinned(knn_idx, (B, N, 3), S, "knn_idx")
                    near = torch.gather(xyz1.float(), 1, idx.reshape(B, N * 3, 1).expand(-1, -1, 3)).view(B, N, 3, 3)
                    dist = ((xyz2.float().unsqueeze(2) - near) ** 2).sum(-1)
        if chosen is not None:
            chosen.append(idx)
        return Fh.interp3_add(feats1, feats2, None if idx is None else idx.to(torch.int32), dist)


class Backbone(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        npoints, nblocks, nneighbor, n_c, d_points = cfg.num_point, cfg.nblocks, cfg.nneighbor, cfg.num_class, cfg.input_dim
        self.fc1 = nn.Sequential(
            nn.Linear(d_points, 32),
            nn.ReLU(),
            nn.Linear(32, 32)
        )
        self.transformer1 = TransformerBlock(32, cfg.transformer_dim, nneighbor)
        self.transition_downs = nn.ModuleList()
        self.transformers = nn.ModuleList()
        for i in range(nblocks):
            channel = 32 * 2 ** (i + 1)
            self.transition_downs.append(TransitionDown(npoints // 4 ** (i + 1), nneighbor, [channel // 2 + 3, channel, channel]))
            self.transformers.append(TransformerBlock(channel, cfg.transformer_dim, nneighbor))
        self.nblocks = nblocks

    def check_levels(self, N, up):
        """the refusals of a forward on clouds of N points, before anything is launched"""
        for td in self.transition_downs:
            _check_down(td.sa.nsample, td.sa.npoint, N)
            N = td.sa.npoint
            if up:
                _check_up(N)

    def _block(self, blk, xyz, points, level, graph, used):
        if used.block_knn[level] is None:
            pinned = None if graph is None else graph.block_knn[level]
            used.block_knn[level] = blk.neighbours(xyz) if pinned is None else pinned
        return blk(xyz, points, knn_idx=used.block_knn[level])[0]

    @flushing_forward
    def forward(self, x, graph=None, used=None):
        """x [B,N,d_points] (coordinates first) -> points [B,N_last,32 * 2^nblocks], [(xyz, points) per level].  `used`: the PyramidGraph
        this forward fills with what it searched or was handed."""
        if used is None:
            self.check_levels(x.shape[1], up=False)
            used = PyramidGraph(self.nblocks)
        _lib.load()
        _lib.require_gpu(x)
        B, N, d = x.shape
        x = x.float()
        xyz = x[..., :3].detach()
        points = _stack(x.reshape(B * N, d), self.fc1).view(B, N, -1)
        points = self._block(self.transformer1, xyz, points, 0, graph, used)

        xyz_and_feats = [(xyz, points)]
        for i in range(self.nblocks):
            chosen = []
            xyz, points = self.transition_downs[i](xyz, points, fps_idx=None if graph is None else graph.fps_idx[i],
                                                   knn_idx=None if graph is None else graph.down_knn[i], chosen=chosen)
            used.fps_idx[i], used.down_knn[i] = chosen[0]
            points = self._block(self.transformers[i], xyz, points, i + 1, graph, used)
            xyz_and_feats.append((xyz, points))
        return points, xyz_and_feats


def _mean_rows(points):
    B, N, C = points.shape
    return Fh.cloud_mean(points.reshape(B * N, C), B, N)


def _decode(model, points, xyz_and_feats, graph, used):
    """fc2, transformer2 and the TransitionUp / TransformerBlock ladder shared by PointTransformerSeg and PointTransformerDef -> the
    finest level's features [B,N,32]"""
    bb, nb = model.backbone, model.nblocks
    xyz = xyz_and_feats[-1][0]
    B, S, C = points.shape
    points = bb._block(model.transformer2, xyz, _stack(points.reshape(B * S, C), model.fc2).view(B, S, C), nb, graph, used)
    for i in range(nb):
        chosen = []
        points = model.transition_ups[i](xyz, points, xyz_and_feats[- i - 2][0], xyz_and_feats[- i - 2][1],
                                         knn_idx=None if graph is None else graph.up_knn[i], chosen=chosen)
        used.up_knn[i] = chosen[0]
        xyz = xyz_and_feats[- i - 2][0]
        points = bb._block(model.transformers[i], xyz, points, nb - 1 - i, graph, used)
    return points


def _begin(model, x, up):
    model.backbone.check_levels(x.shape[1], up=up)
    _lib.load()
    _lib.require_gpu(x)
    return PyramidGraph(model.backbone.nblocks)


def _done(used):
    if _graph_record is not None:
        _graph_record.graph = used


class PointTransformerCls(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.backbone = Backbone(cfg)
        npoints, nblocks, nneighbor, n_c, d_points = cfg.num_point, cfg.model.nblocks, cfg.model.nneighbor, cfg.num_class, cfg.input_dim
        self.fc2 = nn.Sequential(
            nn.Linear(32 * 2 ** nblocks, 256),
            nn.ReLU(),
            nn.Linear(256, 64),
            nn.ReLU(),
            nn.Linear(64, n_c)
        )
        self.nblocks = nblocks

    @flushing_forward
    def forward(self, x, graph=None):
        used = _begin(self, x, up=False)
        points, _ = self.backbone(x, graph=graph, used=used)
        res = _stack(_mean_rows(points), self.fc2)
        _done(used)
        return res


class PointTransformerSeg(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.backbone = Backbone(cfg)
        npoints, nblocks, nneighbor, n_c, d_points = cfg.num_point, cfg.model.nblocks, cfg.model.nneighbor, cfg.num_class, cfg.input_dim
        self.fc2 = nn.Sequential(
            nn.Linear(32 * 2 ** nblocks, 512),
            nn.ReLU(),
            nn.Linear(512, 512),
            nn.ReLU(),
            nn.Linear(512, 32 * 2 ** nblocks)
        )
        self.transformer2 = TransformerBlock(32 * 2 ** nblocks, cfg.model.transformer_dim, nneighbor)
        self.nblocks = nblocks
        self.transition_ups = nn.ModuleList()
        self.transformers = nn.ModuleList()
        for i in reversed(range(nblocks)):
            channel = 32 * 2 ** i
            self.transition_ups.append(TransitionUp(channel * 2, channel, channel))
            self.transformers.append(TransformerBlock(channel, cfg.model.transformer_dim, nneighbor))

        self.fc3 = nn.Sequential(
            nn.Linear(32, 64),
            nn.ReLU(),
            nn.Linear(64, 64),
            nn.ReLU(),
            nn.Linear(64, n_c)
        )

    @flushing_forward
    def forward(self, x, graph=None):
        used = _begin(self, x, up=True)
        points, xyz_and_feats = self.backbone(x, graph=graph, used=used)
        points = _decode(self, points, xyz_and_feats, graph, used)
        B, N, C = points.shape
        res = _stack(points.reshape(B * N, C), self.fc3).view(B, N, -1)
        _done(used)
        return res


class PointTransformerDef(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        from .Models import RegionReconstruction
        self.backbone = Backbone(cfg)
        npoints, nblocks, nneighbor, n_c, d_points = cfg.num_point, cfg.nblocks, cfg.nneighbor, cfg.num_class, cfg.input_dim
        self.fc2 = nn.Sequential(
            nn.Linear(32 * 2 ** nblocks, 512),
            nn.ReLU(),
            nn.Linear(512, 512),
            nn.ReLU(),
            nn.Linear(512, 32 * 2 ** nblocks)
        )
        self.transformer2 = TransformerBlock(32 * 2 ** nblocks, cfg.transformer_dim, nneighbor)
        self.nblocks = nblocks
        self.transition_ups = nn.ModuleList()
        self.transformers = nn.ModuleList()
        for i in reversed(range(nblocks)):
            channel = 32 * 2 ** i
            self.transition_ups.append(TransitionUp(channel * 2, channel, channel))
            self.transformers.append(TransformerBlock(channel, cfg.transformer_dim, nneighbor))

        self.cls_head_finetune = nn.Sequential(
            nn.Linear(32 * 2 ** nblocks, 256),
            nn.ReLU(),
            nn.Linear(256, 64),
            nn.ReLU(),
            nn.Linear(64, n_c)
        )
        self.DefRec = RegionReconstruction(cfg, 32 + 512)
        self.build_loss_func()

    def build_loss_func(self):
        self.loss_ce = nn.CrossEntropyLoss()

    def get_loss_acc(self, ret, gt):
        loss = self.loss_ce(ret, gt.long())
        pred = ret.argmax(-1)
        acc = (pred == gt).sum() / float(gt.size(0))
        return loss, acc * 100

    @flushing_forward
    def forward(self, x, activate_DefRec=False, graph=None):
        if activate_DefRec and self.DefRec.conv1.in_channels != 32 + 32 * 2 ** self.nblocks:
            # (the reference fails inside DefRec's first convolution: its 32 + 512 input channels fit nblocks = 4 only)
            raise ValueError("activate_DefRec: DefRec reads 32 + 512 channels, nblocks=%d gives 32 + %d" % (self.nblocks, 32 * 2 ** self.nblocks))
        used = _begin(self, x, up=bool(activate_DefRec))
        num_points = x.size(1)
        points, xyz_and_feats = self.backbone(x, graph=graph, used=used)
        global_feature = _mean_rows(points)
        if not activate_DefRec:
            res = _stack(global_feature, self.cls_head_finetune)
            _done(used)
            return res
        points = _decode(self, points, xyz_and_feats, graph, used)
        B = points.shape[0]
        ret = self.DefRec.rows(points.reshape(B * num_points, -1), global_feature, B, num_points)
        _done(used)
        return ret
