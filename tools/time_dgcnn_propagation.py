"""Time DGCNN_Propagation (mlsp_amd/propagation.py on csrc/gnedge.hip) against the stock-torch restatement of the reference
(tests/dgprop_restatement.py, fp32, unfolded: gather, concatenate, 1x1 conv, group_norm, leaky_relu, max) on the same GPU in the same
process -- the only comparator there is.  Needs an MI355X; there is no CPU path.

    python tools/time_dgcnn_propagation.py [--out profiles/dgcnn_propagation_timing.jsonl]

Shape: B = 32, the reference's widths (384 / 512), k = 4, the two (G, N) the model uses: (64, 256) and (256, 512).  A step is forward +
backward of (out * R).sum() with gradients to f, f_q and every parameter, the kNN of both graphs included on both sides.  Per side and
shape: five blocks of --iters steps between HIP events, the two sides alternating block by block after a warm-up of both; the median block
over its steps is the figure, the spread (min, max) is printed next to it.  Device launches per step: kernel events of one profiled step
(a run of its own, outside the timed blocks).  Peak memory: torch.cuda.max_memory_allocated over one step, above what the inputs and
parameters hold.  One JSON line per (shape, side)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dgprop_restatement as R  # noqa: E402
from mlsp_amd.propagation import DGCNN_Propagation  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    B, k = 32, 4
    lines = []
    for G, N in ((64, 256), (256, 512)):
        g = torch.Generator().manual_seed(G + N)
        m = DGCNN_Propagation(k=k).to(dev)
        with torch.no_grad():
            for layer in (m.layer1, m.layer2):
                layer[1].weight.copy_(torch.randn(layer[1].weight.shape, generator=g))
                layer[1].bias.copy_(0.3 * torch.randn(layer[1].bias.shape, generator=g))
        coor, coor_q = torch.randn(B, 3, G, generator=g).to(dev), torch.randn(B, 3, N, generator=g).to(dev)
        f = torch.randn(B, 384, G, generator=g).to(dev).requires_grad_(True)
        f_q = torch.randn(B, 384, N, generator=g).to(dev).requires_grad_(True)
        Rw = torch.randn(B, 384, N, generator=g).to(dev)
        params = dict(m.named_parameters())

        def ours():
            out = m(coor, f, coor_q, f_q)
            (out * Rw).sum().backward()
            return out

        def stock():
            with torch.no_grad():
                q = coor_q.transpose(1, 2)
                idx1, idx2 = R.knn(k, coor.transpose(1, 2), q)[0], R.knn(k, q, q)[0]
            out = R.forward(params, coor, f, coor_q, f_q, idx1, idx2, dtype=torch.float32)
            (out * Rw).sum().backward()
            return out

        def clear():
            f.grad = f_q.grad = None
            m.zero_grad(set_to_none=True)

        sides = {"mlsp_amd": ours, "stock_torch": stock}
        outs = {}
        for name, fn in sides.items():                      # warm-up, and the two sides agree
            for _ in range(3):
                clear()
                outs[name] = fn().detach()
        torch.cuda.synchronize()
        agree = float((outs["mlsp_amd"] - outs["stock_torch"]).abs().max() / outs["stock_torch"].abs().max())
        times = {name: [] for name in sides}
        for _ in range(a.blocks):
            for name, fn in sides.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    clear()
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.iters)
        for name, fn in sides.items():
            clear()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            clear()
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
            lines.append({"shape": {"B": B, "G": G, "N": N, "k": k, "in_dim": 384, "mid_dim": 512}, "side": name,
                          "ms_per_step_median": round(statistics.median(times[name]), 4), "ms_per_step_min": round(min(times[name]), 4),
                          "ms_per_step_max": round(max(times[name]), 4), "blocks": a.blocks, "iters_per_block": a.iters,
                          "device_launches_per_step": launches, "peak_step_memory_MiB": round(peak / 2 ** 20, 1),
                          "out_distance_between_sides": agree})
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
