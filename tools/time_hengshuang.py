"""Times forward + backward of PointTransformerCls and PointTransformerDef (mlsp_amd/hengshuang_model.py) at B=32, num_point 1024,
nblocks 4, nneighbor 16, transformer_dim 512 on the GPU box in the default product mode, and the same models restated with stock torch
ops (tests/hengshuang_restatement.py, fp32, handed the build's own graph) on the same GPU -- the only comparator there is.  HIP events,
warm-up, median of five blocks of `--steps` steps; kernel launches per step (torch.profiler) and peak memory.  Also the per-stage split
of the build (the blocks by level, every TransitionDown and TransitionUp, the heads) and functional.interp3_add / cloud_mean alone against
the torch ops they replace.  No threshold.

    python tools/time_hengshuang.py [--timeout 500]

The process ends itself after --timeout seconds (SIGALRM) whatever state it is in."""
import argparse
import os
import signal
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--timeout", type=int, default=500)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--shape", type=int, nargs=5, default=[32, 1024, 4, 16, 512], metavar=("B", "N", "nblocks", "k", "d"))
ap.add_argument("--no-torch", action="store_true", help="skip the stock-torch comparator")
opt = ap.parse_args()
signal.alarm(opt.timeout)

import torch  # noqa: E402
import hengshuang_restatement as HR  # noqa: E402
from mlsp_amd import functional as Fh, hengshuang_model as hm, pointnet2  # noqa: E402

dev = torch.device("cuda:0")
B, N, nb, k, d = opt.shape
cfg = types.SimpleNamespace(num_point=N, nblocks=nb, nneighbor=k, num_class=10, input_dim=3, transformer_dim=d, dropout=0.0)
cfg.model = cfg
x = torch.randn(B, N, 3, generator=torch.Generator().manual_seed(0)).to(dev)
start = torch.zeros(B, dtype=torch.long, device=dev)


def measure(name, step, launches=True):
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(opt.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / opt.steps)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    print("%-52s %9.3f ms (median of 5 x %d; min %.3f max %.3f), peak %.2f GiB"
          % (name, sorted(times)[2], opt.steps, min(times), max(times), peak), flush=True)
    if launches:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
        print("%-52s %d device launches per step" % (name, n), flush=True)


print("Point Transformer B=%d num_point=%d nblocks=%d nneighbor=%d transformer_dim=%d, gemm_precision %s" % (B, N, nb, k, d, Fh.gemm_precision.current),
      flush=True)
models = {}
for kind, cls, kw in (("cls", hm.PointTransformerCls, {}), ("def", hm.PointTransformerDef, {"activate_DefRec": True})):
    torch.manual_seed(0)
    model = cls(cfg).to(dev).train()
    for td in model.backbone.transition_downs:
        td.sa.fps_start = start
    models[kind] = model
    params = dict(model.state_dict(keep_vars=True))

    def step_hip(model=model, kw=kw):
        model.zero_grad(set_to_none=True)
        model(x, **kw).square().sum().backward()

    with torch.no_grad(), hm.recorded_graph() as rec:
        model(x, **kw)
    graph = {key: [None if t is None else t.long() for t in getattr(rec.graph, key)] for key in ("fps_idx", "down_knn", "block_knn", "up_knn")}
    measure("HIP build, %s fwd+bwd (searches its graph)" % kind, step_hip)

    def step_pinned(model=model, kw=kw, pg=rec.graph):
        model.zero_grad(set_to_none=True)
        model(x, graph=pg, **kw).square().sum().backward()
    measure("HIP build, %s fwd+bwd, graph handed in" % kind, step_pinned, launches=False)
    if not opt.no_torch:
        def step_torch(model=model, params=params, kind=kind, graph=graph):
            """the restatement computes no index: it is handed the graph (its time is the arithmetic's alone, which favours it)"""
            model.zero_grad(set_to_none=True)
            HR.forward(kind, params, nb, x, graph, kind == "def", True, torch.float32)[0].square().sum().backward()
        measure("stock torch restatement, %s fwd+bwd" % kind, step_torch)

# the stages of the Def build, forward + backward each on detached inputs at their level's shape
model = models["def"]
bb = model.backbone
with torch.no_grad():
    _, lv = bb(x)
lv = [(a.detach(), b.detach()) for a, b in lv]


def stage(name, fn, *inputs):
    leaves = [t.clone().requires_grad_(True) for t in inputs]

    def step():
        model.zero_grad(set_to_none=True)
        fn(*leaves).square().sum().backward()
    measure(name, step, launches=False)


blocks_down = [bb.transformer1] + list(bb.transformers)
blocks_up = [model.transformer2] + list(model.transformers)
for l in range(nb + 1):
    xyz, pts = lv[l]
    stage("stage: backbone block, level %d (%d points, %d ch)" % (l, xyz.shape[1], pts.shape[2]), lambda p, blk=blocks_down[l], xyz=xyz: blk(xyz, p)[0], pts)
    stage("stage: decoder block, level %d" % l, lambda p, blk=blocks_up[nb - l], xyz=xyz: blk(xyz, p)[0], pts)
for i in range(nb):
    xyz, pts = lv[i]
    stage("stage: TransitionDown %d (%d -> %d points)" % (i, xyz.shape[1], lv[i + 1][0].shape[1]), lambda p, td=bb.transition_downs[i], xyz=xyz: td(xyz, p)[1], pts)
for i in range(nb):
    (cx, cp), (fx, fp) = lv[nb - i], lv[nb - 1 - i]
    stage("stage: TransitionUp %d (%d -> %d points)" % (i, cx.shape[1], fx.shape[1]),
          lambda a, b, up=model.transition_ups[i], cx=cx, fx=fx: up(cx, a, fx, b), cp, fp)
top = lv[nb][1]
S, C = top.shape[1], top.shape[2]
stage("stage: cloud mean + cls_head_finetune", lambda p: hm._stack(hm._mean_rows(p), model.cls_head_finetune), top)
stage("stage: fc2 (three Linear layers, level %d)" % nb, lambda p: hm._stack(p.reshape(B * S, C), model.fc2), top)
stage("stage: DefRec head", lambda p, g: model.DefRec.rows(p.reshape(B * N, -1), g, B, N), lv[0][1], torch.randn(B, 32 * 2 ** nb, device=dev))

# the two new ops alone, at the finest TransitionUp's shape and the deepest level's mean, against the torch ops they replace
S1 = lv[1][0].shape[1]
feat, add = torch.randn(B, S1, 32, device=dev, requires_grad=True), torch.randn(B, N, 32, device=dev, requires_grad=True)
idx, dist = pointnet2.knn_point(3, lv[1][0], lv[0][0], return_dist=True)
idx32 = idx.to(torch.int32)


def op_step(fn):
    def step():
        feat.grad = add.grad = None
        fn().square().sum().backward()
    return step


measure("op: interp3_add [%d,%d,32] from %d points fwd+bwd" % (B, N, S1), op_step(lambda: Fh.interp3_add(feat, add, idx32, dist)), launches=False)
measure("op: _Interp3 + torch add (what it replaces)", op_step(lambda: pointnet2._Interp3.apply(feat, idx32, dist) + add), launches=False)
measure("op: the same with stock torch ops", op_step(lambda: HR.interp3_add(feat, add, idx, dist, torch.float32)), launches=False)
pts = torch.randn(B, S, C, device=dev, requires_grad=True)


def mean_step(fn):
    def step():
        pts.grad = None
        fn().square().sum().backward()
    return step


measure("op: cloud_mean [%d,%d,%d] fwd+bwd" % (B, S, C), mean_step(lambda: Fh.cloud_mean(pts.reshape(B * S, C), B, S)), launches=False)
measure("op: torch mean(1)", mean_step(lambda: pts.mean(1)), launches=False)
big = torch.randn(B, N, 512, device=dev, requires_grad=True)
measure("op: cloud_mean [%d,%d,512] fwd+bwd" % (B, N), lambda: (big.__setattr__("grad", None), Fh.cloud_mean(big.reshape(B * N, 512), B, N).square().sum().backward()), launches=False)
measure("op: torch mean(1) at that shape", lambda: (big.__setattr__("grad", None), big.mean(1).square().sum().backward()), launches=False)
