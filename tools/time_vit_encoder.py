"""Times forward + backward of the Point-BERT TransformerEncoder at the reference's shape (B=32, L=65, d=384, 6 heads, depth 12) on the
GPU box, and the same encoder restated with stock torch ops (tests/vit_restatement.py) on the same GPU -- the only comparator there is.
HIP events, median of five blocks of `--steps` steps; kernel launches per step (torch.profiler) and peak memory.  No threshold.

    python tools/time_vit_encoder.py [--timeout 240]

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
ap.add_argument("--shape", type=int, nargs=5, default=[32, 65, 384, 6, 12], metavar=("B", "L", "d", "heads", "depth"))
opt = ap.parse_args()
signal.alarm(opt.timeout)

import torch  # noqa: E402
import vit_restatement as vr  # noqa: E402
from mlsp_amd.vit import TransformerEncoder  # noqa: E402

dev = torch.device("cuda:0")
B, L, d, heads, depth = opt.shape
torch.manual_seed(0)
x = torch.randn(B, L, d).to(dev).requires_grad_(True)
pos = (0.5 * torch.randn(B, L, d)).to(dev).requires_grad_(True)
R = torch.randn(B, L, d).to(dev)
enc = TransformerEncoder(embed_dim=d, depth=depth, num_heads=heads).to(dev)
params = {n: p for n, p in enc.named_parameters()}


def loss_of(out, feats):
    loss = (out * R).sum()
    for f in feats:
        loss = loss + (f * R).sum()
    return loss


def clear():
    enc.zero_grad(set_to_none=True)
    x.grad = pos.grad = None


def step_hip():
    clear()
    loss_of(*enc(x, pos)).backward()


def step_torch():
    clear()
    loss_of(*vr.encoder_forward(params, x, pos, heads, depth, torch.float32)).backward()


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


print("TransformerEncoder B=%d L=%d d=%d heads=%d depth=%d: a [B,H,L,L] tensor would be %.1f MB per block"
      % (B, L, d, heads, depth, B * heads * L * L * 4 / 1e6), flush=True)
measure("HIP attn kernels + pointmlp", step_hip)
measure("stock torch restatement", step_torch)
