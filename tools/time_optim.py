"""Optimizer step time on the DGCNN + heads parameter set (4.55 M trainable parameters, 77 tensors): torch.optim.SGD's default path on GPU
tensors (multi-tensor foreach) against mlsp_amd.optim.FlatSGD (one launch of mlsp_sgd_flat_f32), both as the trainers build them with
`--optimizer SGD` (momentum 0.9, weight decay 5e-5); FlatAdam for comparison.  The gradients come from one trainer-shaped forward + backward
(activate_density_normal_ondef); then only opt.step() is timed, with device events, after warm-up.  Prints one JSON line per optimizer.

  python tools/time_optim.py [--steps 200] [--warmup 20] [--only sgd,flat_sgd,flat_adam]

Launch count and kernel time per step: one optimizer per profiled run, e.g.
  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/time_optim.py --only flat_sgd
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make(name, params):
    from mlsp_amd.optim import FlatAdam, FlatSGD
    if name == "sgd":
        return torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-5)
    if name == "flat_sgd":
        return FlatSGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-5)
    return FlatAdam(params, lr=1e-3, weight_decay=5e-5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--only", default="sgd,flat_sgd,flat_adam")
    a = ap.parse_args()
    import golden_common as gc
    from mlsp_amd import Models
    dev = torch.device("cuda:0")
    for name in a.only.split(","):
        torch.manual_seed(0)
        m = Models.DGCNN(gc.make_args(cuda=True)).to(dev).train()
        opt = make(name, m.parameters())
        x = torch.rand(8, 3, 1024, device=dev) * 2 - 1
        out = m(x, activate_density_normal_ondef=True)
        sum(v.float().sum() for v in out.values()).backward()
        n_grad = sum(p.numel() for p in m.parameters() if p.grad is not None)
        for _ in range(a.warmup):
            opt.step()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            opt.step()
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / a.steps
        print(json.dumps({"optimizer": name, "step_us": round(1e3 * ms, 2), "steps": a.steps, "warmup": a.warmup, "stepped_params": n_grad,
                          "stepped_tensors": sum(1 for p in m.parameters() if p.grad is not None),
                          "flat_steps": getattr(opt, "flat_steps", None), "device": torch.cuda.get_device_name(dev)}), flush=True)


if __name__ == "__main__":
    main()
