"""DGCNN_Propagation of the reference (PointDA/Models.py:289-363), the Point-BERT side's upsampling block, on MI355X.

Same class name, constructor argument, tensor layouts ([B,3,G], [B,C,G], [B,3,N], [B,C,N] -> [B,C,N]) and state_dict keys: the
nn.Conv2d / nn.GroupNorm members of `layer1` / `layer2` hold the parameters only.  A stage of the reference gathers the edge tensor
[f_j - f_i ; f_i] of the k nearest neighbours, runs a 1x1 conv, GroupNorm(4), LeakyReLU(0.2) over every edge and takes the maximum over
the neighbours.  Here the conv is FOLDED: with its weight W = [Wa | Wb] the edge value is u_j + w_i,

    u = pointmlp(f rows, Wa)                 per source point
    w = pointmlp(f_q rows, Wb - Wa)          per query point
    out = gn_edge_max(u, w, idx, ...)        GroupNorm statistics, LeakyReLU and the max over k in csrc/gnedge.hip

so no tensor with an edge axis exists in either direction.  Stage 2 works on the same-set graph of the query points over stage 1's
output; both its products read one operand, so it is ONE GEMM with the stacked weight [Wa ; Wb - Wa].  The weight slices and Wb - Wa are
torch ops on the weight (tiny; autograd carries their gradients).  Indices carry no gradient and coordinates get none (the reference's
no_grad).  No CPU fallback.
"""
import torch
import torch.nn as nn

from . import _lib
from . import functional as Fh
from . import pointnet2


class DGCNN_Propagation(nn.Module):
    def __init__(self, k=16, *, in_dim=384, mid_dim=512):
        super().__init__()
        '''
        K has to be 16
        '''
        self.k = k
        self.layer1 = nn.Sequential(nn.Conv2d(2 * in_dim, mid_dim, kernel_size=1, bias=False),
                                    nn.GroupNorm(4, mid_dim),
                                    nn.LeakyReLU(negative_slope=0.2))
        self.layer2 = nn.Sequential(nn.Conv2d(2 * mid_dim, in_dim, kernel_size=1, bias=False),
                                    nn.GroupNorm(4, in_dim),
                                    nn.LeakyReLU(negative_slope=0.2))

    @staticmethod
    def fps_downsample(coor, x, num_group):
        """coor [B,3,N], x [B,C,N] -> the num_group farthest-point samples of both, starting from point 0 (what pointnet2_ops'
        furthest_point_sample does): ([B,3,num_group], [B,C,num_group])"""
        _lib.require_gpu(coor, x)
        B = coor.shape[0]
        xyz = coor.transpose(1, 2).contiguous()
        fps_idx = pointnet2.farthest_point_sample(xyz, num_group, start=torch.zeros((B,), dtype=torch.long, device=coor.device))
        combined = torch.cat([coor, x], dim=1)
        new = combined.gather(2, fps_idx.unsqueeze(1).expand(-1, combined.shape[1], -1))
        return new[:, :3], new[:, 3:]

    def _stage(self, layer, idx32, fk, fq):
        """fk [B*Nk, Cin] source rows, fq [B*Nq, Cin] query rows (fq is fk: the same-set stage) -> [B*Nq, Cout]"""
        conv, gn, act = layer[0], layer[1], layer[2]
        Cout, Cin = conv.weight.shape[0], conv.weight.shape[1] // 2
        W = conv.weight.view(Cout, 2 * Cin)
        Wa, Wd = W[:, :Cin], W[:, Cin:] - W[:, :Cin]
        if fq is fk:
            uw = Fh.pointmlp(fk, torch.cat([Wa, Wd], dim=0))
            u, w = uw[:, :Cout], uw[:, Cout:]
        else:
            u, w = Fh.pointmlp(fk, Wa.contiguous()), Fh.pointmlp(fq, Wd)
        return Fh.gn_edge_max(u, w, idx32, gn.weight, gn.bias, gn.num_groups, gn.eps, act.negative_slope)

    def forward_rows(self, coor, f, coor_q, f_q):
        """coor [B,G,3], f [B*G, C], coor_q [B,N,3], f_q [B*N, C] (row matrices, point-major) -> [B*N, C]"""
        _lib.load()
        _lib.require_gpu(coor, f, coor_q, f_q)
        B, G, _ = coor.shape
        N = coor_q.shape[1]
        assert f.shape[0] == B * G and f_q.shape[0] == B * N, (coor.shape, f.shape, coor_q.shape, f_q.shape)
        with torch.no_grad():
            idx1 = pointnet2.knn_point(self.k, coor, coor_q).int()
            idx2 = pointnet2.knn_point(self.k, coor_q, coor_q).int()
        h = self._stage(self.layer1, idx1, f.float(), f_q.float())
        return self._stage(self.layer2, idx2, h, h)

    def forward(self, coor, f, coor_q, f_q):
        """ coor, f : B 3 G ; B C G
            coor_q, f_q : B 3 N; B C N
        """
        _lib.load()
        _lib.require_gpu(coor, f, coor_q, f_q)
        B, C, G = f.shape
        N = f_q.shape[2]
        out = self.forward_rows(coor.transpose(1, 2).contiguous(), f.transpose(1, 2).reshape(B * G, C),
                                coor_q.transpose(1, 2).contiguous(), f_q.transpose(1, 2).reshape(B * N, C))
        return out.view(B, N, -1).transpose(1, 2).contiguous()
