"""Per-launch times of the kernels of mlsp_pointmlp_colmax_bwd_f32 from a rocprofv3 kernel trace of the bench step:
    python tools/prof/colmax_bwd_trace.py run_kernel_trace.csv [skip_calls] > profiles/colmax_bwd_<tag>.csv
A call runs from colmax_bwd_coef_kernel to its scatter kernel on one stream.  A step holds two calls, conv5 (Cin 512) and T-Net conv3
(Cin 128): of each pair, the one whose kernels take longer in total is conv5.  One row per (layer, kernel, how many times the kernel
had already run in the call).  skip_calls: calls dropped from the front (warm-up steps), default 10."""
import csv
import re
import sys


def short(name):
    name = re.sub(r"^void ", "", name)
    return re.sub(r"\(.*", "", name)


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    skip = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None
    for r in rows:
        n = short(r["Kernel_Name"])
        if n.startswith("colmax_bwd_coef_kernel"):
            cur = []
        if cur is not None:
            cur.append((n, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
            if n.startswith("colmax_scatter"):
                calls.append(cur); cur = None
    calls = calls[skip:]
    # two calls per step, conv5's backward first: the one whose kernels take longer in total is conv5 (4x the columns)
    layers = {}
    for i in range(0, len(calls) - 1, 2):
        a, b = calls[i], calls[i + 1]
        if sum(t for _, t in a) < sum(t for _, t in b):
            a, b = b, a
        for tag, call in (("conv5_cin512", a), ("tnet_cin128", b)):
            seen = {}
            for n, t in call:
                k = seen.get(n, 0); seen[n] = k + 1
                layers.setdefault((tag, n, k), []).append(t)
    w = csv.writer(sys.stdout)
    w.writerow(["layer", "kernel", "launch_in_call", "calls", "avg_us", "min_us", "max_us"])
    for (tag, n, k), ts in layers.items():
        w.writerow([tag, n, k, len(ts), "%.2f" % (sum(ts) / len(ts)), "%.2f" % min(ts), "%.2f" % max(ts)])


if __name__ == "__main__":
    main()
