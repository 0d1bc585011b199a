"""The Point-BERT PointTransformer of the reference (PointDA/Models.py:365-531) with its Group and Encoder (PointDA/model_utils.py:170-198,
292-336) on MI355X.

Same class names, constructor arguments, tensor layouts and state_dict keys, parameters registered in the reference's order (identical
initialisation under the same seed, `cls_pos` = torch.randn included): the nn.Conv1d / nn.Linear / nn.BatchNorm1d / nn.LayerNorm members
hold the parameters only.  The arithmetic, on row matrices:

    Group       farthest_point_sample (start 0) -> knn_point -> the grouping kernel            [B,G,M,3], [B,G,3]
    Encoder     thin_in (Conv1d(3,128)+BN+ReLU, csrc/token.hip) -> pointmlp -> segmax
                each cat([global.expand, feature]) + conv stage: ONE pointmlp on the per-point half of the weight, the group half as a
                per-group bias (rows_per_group = M): the 512-channel concatenation is never built
                last conv + max over M: pointmlp_segmax (identity BatchNorm), no activated tensor
    model       reduce_dim: pointmlp; pos_embed: thin_in (gelu) + pointmlp; vit.TransformerEncoder; layernorm; token_pool (csrc/token.hip);
                classification head: Linear+ReLU (identity-BN pointmlp), torch's dropout on [B,256], Linear
    DefRec      self.norm on the three fetched features, PointNetFeaturePropagation x2, DGCNN_Propagation x2, propagation_0, then
                RegionReconstruction.rows(f_level_0 rows, concat_f): [B, 3 trans_dim, N] is never built

NEST_FPS: farthest point sampling from point 0 is a prefix code -- the first k samples of a longer run are the k-sample run -- so the
DefRec path samples ONCE, max(512, num_group) points, and hands Group and the two coarser levels their prefixes.

Only encoder_type 'Encoder'.  No CPU fallback.  Not built: Relative_Encoder, Dgcnn_Encoder, Pointnet_Encoder, dropout inside the stack,
gradients with respect to the coordinates.
"""
import torch
import torch.nn as nn

from . import _lib
from . import functional as Fh
from . import pointnet2
from .model_utils import _bn_buffers, flushing_forward
from .propagation import DGCNN_Propagation
from .seg_models import _identity_bn, _linear_act
from .vit import TransformerEncoder

NEST_FPS = True          # one farthest_point_sample per DefRec forward (tests switch it off to compare)


def _fps0(xyz, npoint):
    """the reference's furthest_point_sample: starts at point 0"""
    return pointnet2.farthest_point_sample(xyz, npoint, start=torch.zeros((xyz.shape[0],), dtype=torch.long, device=xyz.device))


def fps(data, number):
    """PointDA/Models.py:16-23.  data [B,N,3] -> the `number` farthest-point samples [B,number,3], starting at point 0"""
    _lib.require_gpu(data)
    return pointnet2.index_points(data, _fps0(data, number))


class Group(nn.Module):
    def __init__(self, num_group, group_size):
        super().__init__()
        if not 1 <= group_size <= 64:
            raise ValueError("group_size=%d: the query-kNN kernel keeps at most 64 neighbours" % group_size)
        self.num_group = num_group
        self.group_size = group_size

    def forward(self, xyz, fps_idx=None):
        '''
            input: B N 3   (fps_idx [B, num_group] int64: centres already sampled from point 0, optional)
            ---------------------------
            output: B G M 3
            center : B G 3
        '''
        _lib.load()
        _lib.require_gpu(xyz)
        B, N, _ = xyz.shape
        G, M = self.num_group, self.group_size
        if M > N or G > N:
            raise ValueError("Group(num_group=%d, group_size=%d) on clouds of %d points" % (G, M, N))
        xyz = xyz.float().contiguous()
        with torch.no_grad():
            if fps_idx is None:
                fps_idx = _fps0(xyz, G)
            assert fps_idx.shape == (B, G), (fps_idx.shape, B, G)
            center = pointnet2.index_points(xyz, fps_idx)
            idx = pointnet2.knn_point(M, xyz, center)
            neighborhood = pointnet2._Group.apply(xyz, center, None, idx).view(B, G, M, 3)
        return neighborhood, center


def _bn_of(bn, training):
    rm, rv = _bn_buffers(bn, training)
    return dict(gamma=bn.weight, beta=bn.bias, run_mean=rm, run_var=rv, training=training, momentum=bn.momentum, eps=bn.eps)


def _w(conv):
    return conv.weight.view(conv.out_channels, conv.in_channels)


class Encoder(nn.Module):
    def __init__(self, encoder_channel):
        super().__init__()
        self.encoder_channel = encoder_channel
        self.first_conv = nn.Sequential(
            nn.Conv1d(3, 128, 1),
            nn.BatchNorm1d(128),
            nn.ReLU(inplace=True),
            nn.Conv1d(128, 256, 1)
        )
        self.addconv = True
        if self.addconv:
            self.add_conv1 = nn.Sequential(
                nn.Conv1d(512, 512, 1),
                nn.BatchNorm1d(512),
                nn.ReLU(inplace=True),
                nn.Conv1d(512, 256, 1)
            )
        self.second_conv = nn.Sequential(
            nn.Conv1d(512, 512, 1),
            nn.BatchNorm1d(512),
            nn.ReLU(inplace=True),
            nn.Conv1d(512, self.encoder_channel, 1)
        )

    def _cat_stage(self, seq, glob, feat, M):
        """seq[0:3] on cat([glob.expand, feat]) (model_utils.py:327-330): the group half of the weight as a per-group bias"""
        Wg, Wf = Fh.split_columns(_w(seq[0]), glob.shape[1])
        gb = Fh.pointmlp(glob, Wg, training=self.training)
        return Fh.pointmlp(feat, Wf, bias=seq[0].bias, gbias=gb, rows_per_group=M, act=Fh.ACT_RELU, **_bn_of(seq[1], self.training))

    def rows(self, X, M):
        """X [R, 3]: the grouped points, M consecutive rows per group -> [R // M, encoder_channel]"""
        c0, c1 = self.first_conv[0], self.first_conv[3]
        h = Fh.thin_in(X, _w(c0), c0.bias, act=Fh.ACT_RELU, **_bn_of(self.first_conv[1], self.training))
        feat = Fh.pointmlp(h, _w(c1), bias=c1.bias)
        glob = Fh.segmax(feat, M)
        if self.addconv:
            h = self._cat_stage(self.add_conv1, glob, feat, M)
            feat = Fh.pointmlp(h, _w(self.add_conv1[3]), bias=self.add_conv1[3].bias)
            glob = Fh.segmax(feat, M)
        h = self._cat_stage(self.second_conv, glob, feat, M)
        last = self.second_conv[3]
        if Fh.pointmlp_segmax_supported(h.shape[0], last.out_channels, M):
            ones, _, rm, rv = _identity_bn(last.out_channels, h.device)      # (the layer's bias rides as the identity BatchNorm's beta)
            return Fh.pointmlp_segmax(h, _w(last), M, gamma=ones, beta=last.bias, run_mean=rm, run_var=rv, training=False, act=Fh.ACT_NONE,
                                      eps=0.0)
        return Fh.segmax(Fh.pointmlp(h, _w(last), bias=last.bias), M)

    @flushing_forward
    def forward(self, point_groups):
        '''
            point_groups : B G N 3
            -----------------
            feature_global : B G C
        '''
        _lib.load()
        _lib.require_gpu(point_groups)
        bs, g, n, _ = point_groups.shape
        return self.rows(point_groups.reshape(bs * g * n, 3).float(), n).view(bs, g, self.encoder_channel)


class PointTransformer(nn.Module):
    def __init__(self, config, **kwargs):
        super().__init__()
        from .Models import RegionReconstruction            # (Models imports this module at its end)
        self.config = config

        self.trans_dim = config.trans_dim
        self.depth = config.depth
        self.drop_path_rate = config.drop_path_rate
        self.cls_dim = config.cls_dim
        self.num_heads = config.num_heads

        self.group_size = config.group_size
        self.num_group = config.num_group
        # grouper
        self.group_divider = Group(num_group=self.num_group, group_size=self.group_size)
        # define the encoder
        self.encoder_dims = config.encoder_dims
        self.encoder_type = config.encoder_type
        if self.encoder_type != 'Encoder':
            raise NotImplementedError("encoder_type=%r: only 'Encoder' is built (not Pointnet_Encoder, Dgcnn_Encoder, Relative_Encoder)"
                                      % (self.encoder_type,))
        self.encoder = Encoder(encoder_channel=self.encoder_dims)
        # bridge encoder and transformer
        self.reduce_dim = nn.Linear(self.encoder_dims, self.trans_dim)

        self.cls_token = nn.Parameter(torch.zeros(1, 1, self.trans_dim))
        self.cls_pos = nn.Parameter(torch.randn(1, 1, self.trans_dim))

        self.pos_embed = nn.Sequential(
            nn.Linear(3, 128),
            nn.GELU(),
            nn.Linear(128, self.trans_dim)
        )

        dpr = [x.item() for x in torch.linspace(0, self.drop_path_rate, self.depth)]
        self.blocks = TransformerEncoder(
            embed_dim=self.trans_dim,
            depth=self.depth,
            drop_path_rate=dpr,
            num_heads=self.num_heads
        )

        self.norm = nn.LayerNorm(self.trans_dim)

        self.cls_head_finetune = nn.Sequential(
            nn.Linear(self.trans_dim * 2, 256),
            nn.ReLU(inplace=True),
            nn.Dropout(0.5),
            nn.Linear(256, self.cls_dim)
        )

        self.build_loss_func()

        ### for deformation reconstruction
        self.propagation_2 = pointnet2.PointNetFeaturePropagation(in_channel=self.trans_dim + 3, mlp=[self.trans_dim * 4, self.trans_dim])
        self.propagation_1 = pointnet2.PointNetFeaturePropagation(in_channel=self.trans_dim + 3, mlp=[self.trans_dim * 4, self.trans_dim])
        self.propagation_0 = pointnet2.PointNetFeaturePropagation(in_channel=self.trans_dim + 3, mlp=[self.trans_dim * 4, self.trans_dim])
        self.dgcnn_pro_1 = DGCNN_Propagation(k=4, in_dim=self.trans_dim, mid_dim=512)
        self.dgcnn_pro_2 = DGCNN_Propagation(k=4, in_dim=self.trans_dim, mid_dim=512)

        self.DefRec = RegionReconstruction(self.config, self.trans_dim * 2 + self.trans_dim)

    def build_loss_func(self):
        self.loss_ce = nn.CrossEntropyLoss()

    def get_loss_acc(self, ret, gt):
        loss = self.loss_ce(ret, gt.long())
        pred = ret.argmax(-1)
        acc = (pred == gt).sum() / float(gt.size(0))
        return loss, acc * 100

    def load_model_from_ckpt(self, bert_ckpt_path):
        ckpt = torch.load(bert_ckpt_path)
        base_ckpt = {k.replace("module.", ""): v for k, v in ckpt['base_model'].items()}
        for k in list(base_ckpt.keys()):
            if k.startswith('transformer_q') and not k.startswith('transformer_q.cls_head'):
                base_ckpt[k[len('transformer_q.'):]] = base_ckpt[k]
            elif k.startswith('base_model'):
                base_ckpt[k[len('base_model.'):]] = base_ckpt[k]
            del base_ckpt[k]
        incompatible = self.load_state_dict(base_ckpt, strict=False)
        if incompatible.missing_keys:
            print('missing_keys', sorted(incompatible.missing_keys))
        if incompatible.unexpected_keys:
            print('unexpected_keys', sorted(incompatible.unexpected_keys))
        print(f'[Transformer] Successful Loading the ckpt from {bert_ckpt_path}')

    def _normed_tokens(self, t, B, L):
        """self.norm(t)[:, 1:] as rows [B*G, C] (Models.py:502)"""
        n = self.norm
        y = Fh.layernorm(t.reshape(B * L, -1), n.weight, n.bias, n.eps)[1]
        return y.view(B, L, -1)[:, 1:].reshape(B * (L - 1), -1)

    @flushing_forward
    def forward(self, pts, activate_DefRec=False):
        _lib.load()
        _lib.require_gpu(pts)
        B, N, _ = pts.shape
        G, M, d = self.num_group, self.group_size, self.trans_dim
        if activate_DefRec:
            if N < 512:
                raise ValueError("activate_DefRec needs at least 512 points per cloud (fps(pts, 512)), got %d" % N)
            if self.depth < 12:
                raise ValueError("activate_DefRec fetches the outputs of blocks 3, 7 and 11: depth %d < 12" % self.depth)
        pts = pts.float().contiguous()
        # divide the point cloud in the same form. This is important
        fps_all = _fps0(pts, max(512, G)) if activate_DefRec and NEST_FPS else None
        neighborhood, center = self.group_divider(pts, fps_idx=None if fps_all is None else fps_all[:, :G].contiguous())
        # encode the input cloud blocks, bridge encoder and transformer
        tokens = self.encoder.rows(neighborhood.view(B * G * M, 3), M)
        tokens = Fh.pointmlp(tokens, self.reduce_dim.weight, bias=self.reduce_dim.bias)
        # add pos embedding
        pe0, pe2 = self.pos_embed[0], self.pos_embed[2]
        pos = Fh.thin_in(center.reshape(B * G, 3), pe0.weight, pe0.bias, act=Fh.ACT_GELU)
        pos = Fh.pointmlp(pos, pe2.weight, bias=pe2.bias)
        # final input: cls token and position in front
        x = torch.cat((self.cls_token.expand(B, -1, -1), tokens.view(B, G, d)), dim=1)
        pos = torch.cat((self.cls_pos.expand(B, -1, -1), pos.view(B, G, d)), dim=1)
        L = G + 1
        # transformer
        x, feature_list = self.blocks(x, pos)
        y = Fh.layernorm(x.reshape(B * L, d), self.norm.weight, self.norm.bias, self.norm.eps)[1]
        concat_f = Fh.token_pool(y, B, L)                                   # [B, 2 d]

        if activate_DefRec:
            feats = [self._normed_tokens(t, B, L) for t in feature_list]    # three [B*G, d]
            if fps_all is not None:
                level_1, level_2 = pointnet2.index_points(pts, fps_all[:, :512]), pointnet2.index_points(pts, fps_all[:, :256])
            else:
                level_1, level_2 = fps(pts, 512), fps(pts, 256)             # [B,512,3], [B,256,3]
            cm = lambda a: a.transpose(1, 2)                                # noqa: E731  (the propagation modules speak [B,C,N])
            c0, c1, c2, c3 = cm(pts), cm(level_1), cm(level_2), cm(center)
            # init the feature by 3nn propagation
            f3 = feats[2]
            f2 = self.propagation_2(c2, c3, c2, cm(feats[1].view(B, G, d)))
            f1 = self.propagation_1(c1, c3, c1, cm(feats[0].view(B, G, d)))
            # bottom up
            f2 = self.dgcnn_pro_2.forward_rows(center, f3, level_2, cm(f2).reshape(B * 256, d))
            f1 = self.dgcnn_pro_1.forward_rows(level_2, f2, level_1, cm(f1).reshape(B * 512, d))
            f0 = self.propagation_0(c0, c1, c0, cm(f1.view(B, 512, d)))     # point-wise feature [B,d,N]
            return self.DefRec.rows(cm(f0).reshape(B * N, d), concat_f, B, N)

        h0, drop, h3 = self.cls_head_finetune[0], self.cls_head_finetune[2], self.cls_head_finetune[3]
        h = _linear_act(concat_f, h0.weight, h0.bias, Fh.ACT_RELU)
        h = torch.nn.functional.dropout(h, drop.p, self.training)
        return Fh.pointmlp(h, h3.weight, bias=h3.bias)
