"""Time the supervised half of a PointSegDA step (mlsp_amd.seg_train.seg_step + backward: csrc/segsup.hip) beside what it replaces -- torch's
F.cross_entropy on the permuted view, logits.max(dim=2), backward, and the trainer's per-cloud metric loop (2 B copies to the host, B
jaccard_score calls; PointSegDA/trainer.py:224-233) -- at the trainer's shapes, in one process, the two alternating block by block.

Wall time: a host clock around a block of calls that ends in a device synchronise (the metric loop synchronises by itself), warm-up first,
median of the blocks and their spread.  Kernel time comes from a run of its own under the profiler, one path per run:

    python tools/time_seg_step.py --out profiles/seg_step_timing.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/ours -o run -- python tools/time_seg_step.py --only ours --iters 200
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT/parent -o run -- python tools/time_seg_step.py --only parent --iters 200
    python tools/time_seg_step.py --kernel-stats OUT/ours/run_kernel_stats.csv OUT/parent/run_kernel_stats.csv --iters 200 --append profiles/seg_step_timing.txt
"""
import argparse
import csv
import os
import re
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((16, 2048, 8), (32, 1024, 8))
WARM = 10


def macro_jaccard():
    """the trainer's jaccard_score(average='macro'); without scikit-learn the numpy restatement of it (tests/segsup_restatement.py)"""
    try:
        from sklearn.metrics import jaccard_score
        return (lambda y, p: jaccard_score(y, p, average="macro")), "sklearn.metrics.jaccard_score"
    except ImportError:
        import segsup_restatement as sr
        return (lambda y, p: sr.cloud_metrics(y, p, 64)[0]), "numpy restatement of jaccard_score (scikit-learn not installed)"


def make(B, N, C, dev):
    g = torch.Generator().manual_seed(B + N)
    logits = (3 * torch.randn(B, N, C, generator=g)).to(dev).requires_grad_(True)
    labels = torch.randint(0, C, (B, N), generator=g).to(dev)
    return logits, labels


def paths(logits, labels, jaccard):
    from mlsp_amd import seg_train

    def ours():
        logits.grad = None
        loss, preds, miou, acc = seg_train.seg_step(logits, labels)
        loss.backward()
        return loss, miou, acc

    def parent_device():
        logits.grad = None
        loss = torch.nn.functional.cross_entropy(logits.permute(0, 2, 1), labels)
        preds = logits.max(dim=2)[1]
        loss.backward()
        return loss, preds

    def host_metrics(preds):
        """the work of the replaced metric code, cloud by cloud: two device-to-host copies, one macro Jaccard, one mean of equality"""
        iou_total, hit_total = 0.0, 0.0
        for want_row, got_row in zip(labels, preds):
            want, got = want_row.cpu().numpy(), got_row.cpu().numpy()
            iou_total += jaccard(want, got)
            hit_total += float((want == got).mean())
        return iou_total, hit_total

    def parent():
        loss, preds = parent_device()
        return loss, host_metrics(preds)

    def ours_to_host():                                          # what a trainer that logs every step pays on top: one copy of [B] + [B]
        loss, miou, acc = ours()
        return loss, torch.stack((miou, acc)).cpu()
    return dict(ours=ours, ours_to_host=ours_to_host, parent_device=parent_device, parent=parent)


def block(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps                # us per call


def kernel_table(path, iters):
    """-> (us per iteration, launches per iteration, [(name, calls, us)]) of the kernels that ran once per iteration or more"""
    rows = []
    for r in csv.DictReader(open(path)):
        calls = int(r["Calls"])
        if calls < iters:                                       # set-up kernels (random inputs, the copies' fills)
            continue
        name = re.sub(r"at::native::\(anonymous namespace\)::|at::native::", "", r["Name"]).replace("void ", "")
        name = re.sub(r"\(.*", "", name)[:60]
        rows.append((name, calls / iters, int(r["TotalDurationNs"]) / iters / 1e3))
    return sum(r[2] for r in rows), sum(r[1] for r in rows), sorted(rows, key=lambda r: -r[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--only", choices=("ours", "parent"), default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--kernel-stats", nargs=2, default=None, metavar=("OURS_CSV", "PARENT_CSV"))
    args = ap.parse_args()
    lines = []
    if args.kernel_stats:
        lines.append("kernel time per iteration (rocprofv3 --kernel-trace --stats, one run per path, %d iterations of each shape; both shapes "
                     "averaged: %s)" % (args.iters, ", ".join("B %d N %d C %d" % s for s in SHAPES)))
        for tag, path in zip(("seg_step + backward", "F.cross_entropy + max(dim=2) + backward (no metric loop: it runs no kernel)"), args.kernel_stats):
            tot, n, rows = kernel_table(path, args.iters * len(SHAPES))
            lines.append("  %s: %.1f us in %.1f launches per iteration of one shape" % (tag, tot, n))
            lines += ["    %-60s %5.1f x %7.2f us = %7.2f us" % (name, c, t / c, t) for name, c, t in rows]
    else:
        dev = torch.device("cuda:0")
        jaccard, jname = macro_jaccard()
        if args.only:
            for B, N, C in SHAPES:
                logits, labels = make(B, N, C, dev)
                fn = paths(logits, labels, jaccard)["ours" if args.only == "ours" else "parent_device"]
                for _ in range(args.iters):
                    fn()
            torch.cuda.synchronize()
            return
        lines.append("supervised segmentation step: loss + predictions + per-cloud mIoU / accuracy + backward to the logits; %s; wall us per call, "
                     "median of %d blocks of %d calls [min .. max], the paths alternating block by block; metric loop: %s"
                     % (torch.cuda.get_device_name(0), args.blocks, args.reps, jname))
        for B, N, C in SHAPES:
            logits, labels = make(B, N, C, dev)
            fns = paths(logits, labels, jaccard)
            for f in fns.values():
                for _ in range(WARM):
                    f()
            t = {k: [] for k in fns}
            for _ in range(args.blocks):
                for k, f in fns.items():
                    t[k].append(block(f, args.reps if k != "parent" else max(5, args.reps // 5)))
            what = dict(ours="seg_step + backward, results left on the device", ours_to_host="seg_step + backward + one copy of the metrics to the host",
                        parent_device="F.cross_entropy(permuted view) + max(dim=2) + backward", parent="the same + the trainer's per-cloud metric loop")
            for k in ("ours", "ours_to_host", "parent_device", "parent"):
                lines.append("B %2d N %4d C %d  %-62s %9.1f  [%9.1f .. %9.1f]" % (B, N, C, what[k], np.median(t[k]), min(t[k]), max(t[k])))
            lo, lp = fns["ours"]()[0].item(), fns["parent_device"]()[0].item()
            lines.append("B %2d N %4d C %d  loss %.7f (torch %.7f); whole step: %.2fx; device part alone: %.2fx" % (
                B, N, C, lo, lp, np.median(t["parent"]) / np.median(t["ours_to_host"]), np.median(t["parent_device"]) / np.median(t["ours"])))
    text = "\n".join(lines)
    print(text)
    for path, mode in ((args.out, "w"), (args.append, "a")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, mode) as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
