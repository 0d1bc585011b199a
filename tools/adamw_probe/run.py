"""Lowering probe for the AdamW decay of mlsp_adam_flat_groups_f32 (csrc/optim.hip): one torch._fused_adamw_ step (what
torch.optim.AdamW(fused=True) runs) on 4 Mi random elements in several configurations, against tools/adamw_probe/probe.hip with the
decay `param -= lr * weight_decay * param` uncontracted (mode 0) and contracted into one double fma (mode 1).  Prints the number of
differing elements of param / exp_avg / exp_avg_sq per configuration and mode; the committed output is profiles/adamw_lowering_probe.txt.

  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC tools/adamw_probe/probe.hip -o build/adamw_probe.so
  python tools/adamw_probe/run.py build/adamw_probe.so
"""
import ctypes
import sys

import torch

lib = ctypes.CDLL(sys.argv[1] if len(sys.argv) > 1 else "build/adamw_probe.so")
D, P = ctypes.c_double, ctypes.c_void_p
dev = torch.device("cuda:0")
n = 1 << 22
gen = torch.Generator(device=dev).manual_seed(0)
p0 = torch.randn(n, device=dev, generator=gen) * 0.05
g0 = torch.randn(n, device=dev, generator=gen) * 0.01
m0 = torch.randn(n, device=dev, generator=gen) * 0.01
v0 = torch.rand(n, device=dev, generator=gen) * 1e-4

# (name, lr, beta1, beta2, weight_decay, eps, step)
CONFIGS = [("torch defaults (wd 1e-2)", 1e-3, 0.9, 0.999, 1e-2, 1e-8, 7),
           ("cosine lr, wd 5e-2", 7.3e-4, 0.9, 0.999, 5e-2, 1e-8, 3),
           ("large decay", 1.1e-2, 0.8, 0.99, 0.3, 1e-6, 120),
           ("no decay", 1e-3, 0.9, 0.999, 0.0, 1e-8, 7)]

print("# tools/adamw_probe: one AdamW step on %d elements, the decay uncontracted (mode 0) / one double fma (mode 1), vs torch._fused_adamw_ "
      "(torch %s, %s)." % (n, torch.__version__, torch.cuda.get_device_name(dev)))
for name, lr, b1, b2, wd, eps, step in CONFIGS:
    pt, mt, vt = p0.clone(), m0.clone(), v0.clone()
    st = torch.full((), float(step), device=dev)              # (torch.optim increments the step before it calls the fused kernel)
    torch._fused_adamw_([pt], [g0.clone()], [mt], [vt], [], [st], lr=lr, beta1=b1, beta2=b2, weight_decay=wd, eps=eps, amsgrad=False,
                        maximize=False)
    print("## %s: lr %g betas (%g, %g) weight_decay %g eps %g step %d" % (name, lr, b1, b2, wd, eps, step))
    for mode in range(2):
        p, m, v = p0.clone(), m0.clone(), v0.clone()
        rc = lib.run_probe(P(p.data_ptr()), P(g0.data_ptr()), P(m.data_ptr()), P(v.data_ptr()), n, D(lr), D(b1), D(b2), D(wd), D(eps), step, mode)
        print("mode %d rc %d  param != %7d  exp_avg != %7d  exp_avg_sq != %7d"
              % (mode, rc, (p != pt).sum().item(), (m != mt).sum().item(), (v != vt).sum().item()))
