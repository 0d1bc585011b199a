"""Times forward + backward of one vector-attention TransformerBlock at B=32, N=1024, k=16, d_points=32, d_model=512 on the GPU box, and
the same block restated with stock torch ops (tests/vecattn_restatement.py) on the same GPU and the same neighbour indices -- the only
comparator there is.  HIP events, median of five blocks of `--steps` steps; kernel launches per step (torch.profiler) and peak memory.

    python tools/time_transformer_block.py [--timeout 240]

The process ends itself after --timeout seconds (SIGALRM) whatever state it is in."""
import argparse
import os
import signal
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--timeout", type=int, default=240)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--shape", type=int, nargs=5, default=[32, 1024, 16, 32, 512], metavar=("B", "N", "k", "d_points", "d_model"))
opt = ap.parse_args()
signal.alarm(opt.timeout)

import torch  # noqa: E402
import vecattn_restatement as vr  # noqa: E402
from mlsp_amd.transformer import TransformerBlock  # noqa: E402

dev = torch.device("cuda:0")
B, N, k, d_points, d = opt.shape
torch.manual_seed(0)
xyz = (torch.rand(B, N, 3) * 2 - 1).to(dev)
feat = torch.randn(B, N, d_points).to(dev).requires_grad_(True)
R = torch.randn(B, N, d_points).to(dev)
blk = TransformerBlock(d_points, d, k).to(dev)
idx = blk.neighbours(xyz)
params = {n: p for n, p in blk.named_parameters()}


def step_hip():
    blk.zero_grad(set_to_none=True)
    feat.grad = None
    out, _ = blk(xyz, feat, knn_idx=idx)
    (out * R).sum().backward()


def step_torch():
    blk.zero_grad(set_to_none=True)
    feat.grad = None
    out, _ = vr.block_forward(params, xyz, feat, idx, torch.float32)
    (out * R).sum().backward()


def measure(name, step):
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
    print("%-28s fwd+bwd %8.2f ms (median of 5 x %d; min %.2f max %.2f), peak %.2f GiB"
          % (name, sorted(times)[2], opt.steps, min(times), max(times), peak), flush=True)
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    launches = sum(e.count for e in prof.key_averages() if e.device_type == torch.autograd.DeviceType.CUDA)
    print("%-28s %d device launches per step" % (name, launches), flush=True)


print("TransformerBlock B=%d N=%d k=%d d_points=%d d_model=%d: E*d*4 = %.2f GB per edge tensor" % (B, N, k, d_points, d, B * N * min(k, N) * d * 4 / 1e9),
      flush=True)
measure("HIP edge kernels + pointmlp", step_hip)
measure("stock torch restatement", step_torch)
