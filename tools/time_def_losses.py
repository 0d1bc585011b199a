"""Times the index-matched deformed-region losses (mlsp_amd/csrc/def_loss.hip) at B=32, N=1024 and B=16, N=2048, next to the masked
Chamfer direction (chamfer_dir_fwd_kernel) on the same clouds.  Run under `rocprofv3 --kernel-trace --stats -- python tools/time_def_losses.py`
for per-kernel times; the wall-clock figures printed here include the launches."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse  # noqa: E402
import torch  # noqa: E402
from mlsp_amd import mlsp, pc_utils  # noqa: E402

dev = torch.device("cuda:0")
NC, ITERS = 16, 20
args = argparse.Namespace(Density_normal_defpart=False, normal_pred_weight=0.5, Density_weight=0.05, density_num_class=NC)
lookup = torch.Tensor(pc_utils.region_mean(3)).to(dev)
for B, N in ((32, 1024), (16, 2048)):
    g = torch.Generator().manual_seed(0)
    gold = ((torch.rand(B, 3, N, generator=g) * 2 - 1) * 0.8).to(dev)
    x, mask = mlsp.deform_input(gold.clone(), lookup, 'volume_based_voxels', dev)
    pred = (x.permute(0, 2, 1) + 0.02 * torch.randn(B, N, 3, device=dev)).contiguous()
    normal = torch.randn(B, N, 3, device=dev, requires_grad=True)
    nlab = torch.randn(B, N, 3, device=dev)
    pvec = torch.softmax(torch.randn(B * N, NC, device=dev), 1).requires_grad_(True)
    dens = (torch.rand(B * N, device=dev) * 30).requires_grad_(True)
    dlab = torch.softmax(torch.randn(B * N, NC, device=dev), 1)
    dval = (torch.rand(B, N, device=dev) * 30).round()
    logits = {"Normal": normal, "density": pvec, "density_mse": dens}

    def step():
        idx = mlsp.findindexs(pred, gold, mask)
        loss = mlsp.calc_def_normal_loss(args, logits, nlab, mask, idx, dev)
        kl, mae = mlsp.deform_densityloss(args, logits, dlab, dval, mask, idx, dev)
        (loss + kl + mae).backward()
        mlsp.chamfer_distance(pred, gold.permute(0, 2, 1), mask.permute(0, 2, 1))     # chamfer_dir_fwd_kernel, same shape
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(ITERS):
        step()
    torch.cuda.synchronize()
    print("B=%d N=%d: %.1f us per findindexs + both losses fwd+bwd + one Chamfer direction" % (B, N, (time.perf_counter() - t0) / ITERS * 1e6))
