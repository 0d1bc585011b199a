"""Times forward + backward of the Point-BERT PointTransformer (mlsp_amd/pointbert.py) at the reference's shape (B=32, N=1024, G=64, M=32,
trans_dim 384, depth 12, 6 heads) on the GPU box, both paths, and the same model restated with stock torch ops
(tests/pointbert_restatement.py, fp32, fed the build's own indices) on the same GPU -- the only comparator there is.  HIP events, warm-up,
median of five blocks of `--steps` steps; kernel launches per step (torch.profiler) and peak memory.  Also the per-stage split of the
build (Group, Encoder, transformer stack, the rest of each path) and the DefRec path with NEST_FPS off.  No threshold.

    python tools/time_point_transformer.py [--timeout 500]

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
ap.add_argument("--shape", type=int, nargs=7, default=[32, 1024, 64, 32, 384, 12, 6], metavar=("B", "N", "G", "M", "d", "depth", "heads"))
opt = ap.parse_args()
signal.alarm(opt.timeout)

import torch  # noqa: E402
import pointbert_restatement as PR  # noqa: E402
from mlsp_amd import functional as Fh, pointbert, pointnet2  # noqa: E402

dev = torch.device("cuda:0")
B, N, G, M, d, depth, heads = opt.shape
cfg = types.SimpleNamespace(trans_dim=d, depth=depth, drop_path_rate=0.0, cls_dim=10, num_heads=heads, group_size=M, num_group=G,
                            encoder_dims=256, encoder_type="Encoder", dropout=0.0, model="PointTransformer")
torch.manual_seed(0)
model = pointbert.PointTransformer(cfg).to(dev).train()
model.cls_head_finetune[2].p = 0.0
pts = torch.randn(B, N, 3).to(dev)
params = dict(model.state_dict(keep_vars=True))


def graph_of(defrec):
    g = {"fps_g": pointbert._fps0(pts, G)}
    center = pointnet2.index_points(pts, g["fps_g"])
    g["knn_group"] = pointnet2.knn_point(M, pts, center)
    if defrec:
        g["fps_512"], g["fps_256"] = pointbert._fps0(pts, 512), pointbert._fps0(pts, 256)
        l1, l2 = pointnet2.index_points(pts, g["fps_512"]), pointnet2.index_points(pts, g["fps_256"])
        for key, (ref, qry) in (("nn3_2", (center, l2)), ("nn3_1", (center, l1)), ("nn3_0", (l1, pts))):
            g[key] = pointnet2.knn_point(3, ref, qry, return_dist=True)
        g["pro2"] = (pointnet2.knn_point(4, center, l2), pointnet2.knn_point(4, l2, l2))
        g["pro1"] = (pointnet2.knn_point(4, l2, l1), pointnet2.knn_point(4, l1, l1))
    return g


def step_hip(defrec):
    model.zero_grad(set_to_none=True)
    model(pts, activate_DefRec=defrec).square().sum().backward()


def step_torch(defrec, graph):
    """the restatement computes no index: it is handed the graph (its time is the arithmetic's alone, which favours it)"""
    model.zero_grad(set_to_none=True)
    PR.forward(params, cfg, pts, graph, defrec, True, torch.float32)[0].square().sum().backward()


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
    print("%-44s %8.2f ms (median of 5 x %d; min %.2f max %.2f), peak %.2f GiB"
          % (name, sorted(times)[2], opt.steps, min(times), max(times), peak), flush=True)
    if launches:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
        print("%-44s %d device launches per step" % (name, n), flush=True)


print("PointTransformer B=%d N=%d G=%d M=%d trans_dim=%d depth=%d heads=%d, gemm_precision %s"
      % (B, N, G, M, d, depth, heads, Fh.gemm_precision.current), flush=True)
for defrec in (False, True):
    tag = "DefRec path" if defrec else "classification path"
    measure("HIP build, %s fwd+bwd" % tag, lambda: step_hip(defrec))
    graph = graph_of(defrec)
    measure("stock torch restatement, %s fwd+bwd" % tag, lambda: step_torch(defrec, graph))
pointbert.NEST_FPS = False
measure("HIP build, DefRec path, NEST_FPS off", lambda: step_hip(True), launches=False)
pointbert.NEST_FPS = True

# the stages of the build, forward + backward each on detached inputs
nb, center = model.group_divider(pts)
measure("stage: Group (forward only)", lambda: model.group_divider(pts), launches=False)
rows = nb.view(B * G * M, 3)


def enc_step():
    model.zero_grad(set_to_none=True)
    model.encoder.rows(rows, M).square().sum().backward()


x = torch.randn(B, G + 1, d, device=dev, requires_grad=True)
pos = torch.randn(B, G + 1, d, device=dev, requires_grad=True)


def stack_step():
    model.zero_grad(set_to_none=True)
    out, feats = model.blocks(x, pos)
    (out.square().sum() + sum(f.square().sum() for f in feats)).backward()


measure("stage: Encoder fwd+bwd", enc_step, launches=False)
measure("stage: transformer stack fwd+bwd", stack_step, launches=False)
X3 = torch.randn(B * G * M, 3, device=dev)
c0, bn0 = model.encoder.first_conv[0], model.encoder.first_conv[1]


def thin_step():
    model.zero_grad(set_to_none=True)
    Fh.thin_in(X3, c0.weight.view(128, 3), c0.bias, bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var).square().sum().backward()


def thin_torch():
    model.zero_grad(set_to_none=True)
    PR.thin_in(X3, c0.weight.view(128, 3), c0.bias, bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var, dtype=torch.float32)["H"].square().sum().backward()


measure("op: thin_in [%d,3]->128 BN relu fwd+bwd" % (B * G * M), thin_step, launches=False)
measure("op: the same with stock torch ops", thin_torch, launches=False)
