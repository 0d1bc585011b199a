"""Lowering probe for mlsp_sgd_flat_f32 (csrc/optim.hip): one torch SGD step (torch.optim.sgd.sgd, foreach=True -- the default path of
torch.optim.SGD on GPU tensors) on 4 Mi random elements in several configurations, against tools/sgd_probe/probe.hip under 16 lowerings
(mode bit 1: weight decay contracted to an fma, 2: the dampened momentum add, 4: the nesterov add, 8: the parameter update).  Prints the
number of differing elements of param and momentum buffer per configuration and mode; the committed output is profiles/sgd_lowering_probe.txt.

  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC tools/sgd_probe/probe.hip -o build/sgd_probe.so
  python tools/sgd_probe/run.py build/sgd_probe.so
"""
import ctypes
import sys

import torch
from torch.optim.sgd import sgd

lib = ctypes.CDLL(sys.argv[1] if len(sys.argv) > 1 else "build/sgd_probe.so")
D = ctypes.c_double
dev = torch.device("cuda:0")
n = 1 << 22
gen = torch.Generator(device=dev).manual_seed(0)
p0 = torch.randn(n, device=dev, generator=gen) * 0.05
g0 = torch.randn(n, device=dev, generator=gen) * 0.01
b0 = torch.randn(n, device=dev, generator=gen) * 0.01

# (name, lr, momentum, dampening, weight_decay, nesterov, maximize, first)
CONFIGS = [("trainers (mom 0.9, wd 5e-5)", 7.3e-4, 0.9, 0.0, 5e-5, False, False, False),
           ("trainers, first step", 7.3e-4, 0.9, 0.0, 5e-5, False, False, True),
           ("dampening 0.1", 1.1e-2, 0.9, 0.1, 5e-5, False, False, False),
           ("nesterov", 1.1e-2, 0.9, 0.0, 5e-5, True, False, False),
           ("maximize", 1.1e-2, 0.9, 0.0, 5e-5, False, True, False),
           ("momentum 0", 1.1e-2, 0.0, 0.0, 5e-5, False, False, False),
           ("momentum 0.5, wd 3e-2", 3.7e-1, 0.5, 0.3, 3e-2, False, False, False)]

print("# tools/sgd_probe: one SGD step on %d elements under 16 lowerings vs torch.optim.sgd.sgd(foreach=True) (torch %s, %s)."
      % (n, torch.__version__, torch.cuda.get_device_name(dev)))
print("# mode bits: 1 = weight decay as fma, 2 = dampened momentum add as fma, 4 = nesterov add as fma, 8 = parameter update as fma")
for name, lr, mom, damp, wd, nest, maxi, first in CONFIGS:
    pt, bt = p0.clone(), b0.clone()
    bufs = [None if first else bt] if mom != 0 else []
    sgd([pt], [g0.clone()], bufs, weight_decay=wd, momentum=mom, lr=lr, dampening=damp, nesterov=nest, maximize=maxi,
        has_sparse_grad=False, foreach=True)
    bt = bufs[0] if mom != 0 else bt
    print("## %s: lr %g momentum %g dampening %g weight_decay %g nesterov %d maximize %d first %d" % (name, lr, mom, damp, wd, nest, maxi, first))
    for mode in range(16):
        p, b = p0.clone(), b0.clone()
        rc = lib.run_probe(ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(g0.data_ptr()), ctypes.c_void_p(b.data_ptr()), n, D(lr), D(mom),
                           D(damp), D(wd), int(nest), int(maxi), int(first), mode)
        nb = (b != bt).sum().item() if mom != 0 else 0
        print("mode %2d rc %d  param != %7d  momentum_buffer != %7d" % (mode, rc, (p != pt).sum().item(), nb))
