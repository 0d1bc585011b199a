"""Optimizer step time on the DGCNN + heads parameter set (4.55 M trainable parameters, 77 tensors): torch.optim.SGD's default path on GPU
tensors (multi-tensor foreach) against mlsp_amd.optim.FlatSGD (one launch of mlsp_sgd_flat_groups_f32), both as the trainers build them with
`--optimizer SGD` (momentum 0.9, weight decay 5e-5); FlatAdam for comparison.  `adamw2` / `flat_adamw2`: torch.optim.AdamW(fused=True)
against FlatAdamW over the reference's two parameter groups (utils/optimizer.py add_weight_decay: no decay on 1-D parameters and biases).
The gradients come from one trainer-shaped forward + backward (activate_density_normal_ondef); then only opt.step() is timed, with device
events, after warm-up.  Prints one JSON line per optimizer; with --repeat N every optimizer is timed N times, the legs interleaved
(a, b, c, a, b, c, ...), and a line holds the median and the spread of its N runs.

  python tools/time_optim.py [--steps 200] [--warmup 20] [--repeat 1] [--only sgd,flat_sgd,flat_adam,adamw2,flat_adamw2]

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


def add_weight_decay(model, weight_decay):
    no_decay = [p for n, p in model.named_parameters() if p.requires_grad and (p.dim() == 1 or n.endswith(".bias"))]
    decay = [p for n, p in model.named_parameters() if p.requires_grad and not (p.dim() == 1 or n.endswith(".bias"))]
    return [{"params": no_decay, "weight_decay": 0.0}, {"params": decay, "weight_decay": weight_decay}]


def make(name, model):
    from mlsp_amd.optim import FlatAdam, FlatAdamW, FlatSGD
    params = model.parameters()
    if name == "adamw2":
        return torch.optim.AdamW(add_weight_decay(model, 1e-2), lr=1e-3, fused=True)
    if name == "flat_adamw2":
        return FlatAdamW(add_weight_decay(model, 1e-2), lr=1e-3)
    if name == "sgd":
        return torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-5)
    if name == "flat_sgd":
        return FlatSGD(params, lr=1e-3, momentum=0.9, weight_decay=5e-5)
    return FlatAdam(params, lr=1e-3, weight_decay=5e-5)


def time_steps(opt, steps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        opt.step()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--only", default="sgd,flat_sgd,flat_adam")
    a = ap.parse_args()
    import golden_common as gc
    from mlsp_amd import Models
    dev = torch.device("cuda:0")
    legs = []
    for name in a.only.split(","):
        torch.manual_seed(0)
        m = Models.DGCNN(gc.make_args(cuda=True)).to(dev).train()
        opt = make(name, m)
        x = torch.rand(8, 3, 1024, device=dev) * 2 - 1
        out = m(x, activate_density_normal_ondef=True)
        sum(v.float().sum() for v in out.values()).backward()
        for _ in range(a.warmup):
            opt.step()
        legs.append((name, m, opt, []))
    for _ in range(a.repeat):
        for name, m, opt, us in legs:
            us.append(time_steps(opt, a.steps))
    for name, m, opt, us in legs:
        us = sorted(us)
        print(json.dumps({"optimizer": name, "step_us": round(us[len(us) // 2], 2), "min_us": round(us[0], 2), "max_us": round(us[-1], 2),
                          "repeat": a.repeat, "steps": a.steps, "warmup": a.warmup,
                          "stepped_params": sum(p.numel() for p in m.parameters() if p.grad is not None),
                          "stepped_tensors": sum(1 for p in m.parameters() if p.grad is not None),
                          "groups": len(opt.param_groups), "flat_steps": getattr(opt, "flat_steps", None),
                          "device": torch.cuda.get_device_name(dev)}), flush=True)


if __name__ == "__main__":
    main()
