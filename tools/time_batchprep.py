"""Time the batch preparation (mlsp_amd/data.py prepare_batch, one launch, every stage on) beside `pointnet2.farthest_point_sample`
alone on the already normalised cloud -- the same 1024-step serial loop without prologue and epilogue.  HIP events around blocks of
calls, the two alternating inside one run, warm-up first, median of five blocks and their spread.  Also the numpy restatement's time per
sample on this host's CPU, for context.

    python tools/time_batchprep.py [--out profiles/batchprep_timing.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def block(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps                     # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    from mlsp_amd import data, pointnet2
    import batchprep_restatement as br
    dev = torch.device("cuda:0")
    lines = ["batch preparation, 2048 -> 1024 points, every stage on (unit cube, x rotation, FPS, z rotation, jitter); %s; us per call, "
             "median of 5 blocks of %d calls [min .. max]" % (torch.cuda.get_device_name(0), args.reps)]
    N, S = 2048, 1024
    Rx = data.axis_rotation("x", -np.pi / 2)
    for B in (32, 64):
        g = torch.Generator().manual_seed(B)
        raw = ((torch.rand(B, N, 3, generator=g) * 2 - 1) * torch.tensor([1.0, 0.6, 0.3]) + 0.5).to(dev)
        start = torch.randint(0, N, (B,), generator=g).to(dev)
        noise = torch.randn(B, S, 3, dtype=torch.float64, generator=g).to(dev)
        angles = np.random.RandomState(B).uniform(size=B) * 2 * np.pi
        # the launch alone: flags, matrices and draws prepared once, as a trainer that keeps them on the device would
        counts, flags = np.full(B, N), np.full(B, 7)
        Rpre = torch.from_numpy(np.stack([Rx] * B)).to(dev)
        Rpost = torch.from_numpy(np.stack([data.axis_rotation("z", a) for a in angles])).to(dev)
        st32 = start.to(torch.int32)
        unit = data._run(raw, N, counts, np.zeros(B, dtype=np.int32), None, None, None, None, 0.0, 0.0)[0]

        def fused():
            data._run(raw, S, counts, flags, st32, Rpre, Rpost, noise, 0.01, 0.02)

        def whole():
            data.prepare_batch(raw, S, pre_rotate=Rx, augment=True, start=start, angles=angles, noise=noise)

        def fps():
            pointnet2.farthest_point_sample(unit, S, start=start)
        for f in (fused, whole, fps):
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        t = {"fused": [], "whole": [], "fps": []}
        for _ in range(5):
            t["fused"].append(block(fused, args.reps))
            t["fps"].append(block(fps, args.reps))
            t["whole"].append(block(whole, args.reps))
        med = {k: float(np.median(v)) for k, v in t.items()}
        for k, what in (("fused", "mlsp_batch_prepare_f32 (the launch)"), ("whole", "data.prepare_batch (host glue + launch)"),
                        ("fps", "pointnet2.farthest_point_sample alone")):
            lines.append("B %3d  %-42s %9.1f  [%9.1f .. %9.1f]" % (B, what, med[k], min(t[k]), max(t[k])))
        lines.append("B %3d  fused launch / FPS alone = %.3f;  %.2f us per sample" % (B, med["fused"] / med["fps"], med["fused"] / B))
    x = ((np.random.RandomState(0).uniform(-1, 1, (N, 3)) * [1.0, 0.6, 0.3]) + 0.5).astype(np.float32)
    t0 = time.perf_counter()
    br.chain(x, S, 7, start=5, Rpre=Rx, Rpost=data.axis_rotation("z", 1.0), noise=np.random.RandomState(1).randn(S, 3))
    lines.append("numpy restatement of the same chain, one sample on this host's CPU: %.1f ms" % ((time.perf_counter() - t0) * 1e3))
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
