"""Generate tests/golden/def_losses_*.npz: the index-matched losses on the deformed region of the UNMODIFIED reference
(MLSP/mlsp.py:184-427: findindexs, calc_def_normal_loss, calc_def_density_loss, deform_densityloss), run on the CPU with
autograd.  Build-container only (imports the reference through tools/ref_import.py); the fixtures are numeric arrays.

    python tools/make_golden_def_losses.py

Every case stores its inputs, the reference's index1 / index2, and for Density_normal_defpart in {0, 1} (suffix _dp0 / _dp1):
  normal_loss, d_normal                      calc_def_normal_loss and its gradient w.r.t. logits['Normal']
  kl, mae, dkl_density, dkl_density_mse      deform_densityloss and the gradients of (kl + mae) w.r.t. logits['density'],
                                             logits['density_mse']
and for all in {False, True} (suffix _all0 / _all1):
  cdl_loss, d_cdl_density                    calc_def_density_loss with criterion nn.NLLLoss(reduction='none') (criterion_nll = 1)
                                             on the class labels `density_cls`, and its gradient w.r.t. logits['density'].
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_import  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
NC = 16


def npy(t):
    return t.detach().cpu().numpy()


def make_args(defpart):
    return argparse.Namespace(Density_normal_defpart=defpart, normal_pred_weight=0.5, Density_weight=0.05, density_num_class=NC)


def case(rmlsp, rpc, seed, B, N, dup=False):
    g = torch.Generator().manual_seed(seed)
    X = torch.rand(B, 3, N, generator=g) * 2 - 1                          # [B,3,N] the clean cloud = gold
    if dup:
        # exact distance ties: every point appears twice in both clouds; a crowded centre voxel gives deform_input a region
        X[:, :, :N // 4] = X[:, :, :N // 4] * 0.1
        X[:, :, N // 2:] = X[:, :, :N // 2]
    gold = X.clone()
    lookup = torch.Tensor(rpc.region_mean(3))
    np.random.seed(100 + seed)
    Xd, mask = rmlsp.deform_input(X.clone(), lookup, 'volume_based_voxels', 'cpu', 1)
    pred = Xd.permute(0, 2, 1) + 0.02 * torch.randn(B, N, 3, generator=g)   # a "reconstruction" [B,N,3]
    if dup:
        pred[:, N // 2:] = pred[:, :N // 2]
    normal_pred = torch.randn(B, N, 3, generator=g)
    normal_lab = torch.randn(B, N, 3, generator=g)
    dlogit = torch.randn(B * N, NC, generator=g)
    pvec = torch.softmax(dlogit, dim=1)
    dens = torch.rand(B * N, generator=g) * 30
    cnt = torch.randint(0, 2 * (NC - 1) + 1, (B * N,), generator=g).double()
    lo, hi = torch.floor(cnt / 2).long(), torch.ceil(cnt / 2).long()
    eye = torch.eye(NC)
    dlab = (eye[lo] + eye[hi]) / 2                                          # soft labels as cal_density (MLSP/mlsp.py:262-266)
    dval = cnt.float().reshape(B, N)
    dcls = torch.randint(0, NC, (B * N,), generator=g)
    out = {"pred": npy(pred), "gold": npy(gold), "mask": npy(mask), "normal_pred": npy(normal_pred), "normal_labels": npy(normal_lab),
           "density": npy(pvec), "density_mse": npy(dens), "density_labels": npy(dlab), "density_mse_label": npy(dval),
           "density_cls": npy(dcls), "criterion_nll": np.array(1)}
    index1, index2 = rmlsp.findindexs(pred.clone(), gold.clone(), mask.clone())
    out["index1"], out["index2"] = npy(index1), npy(index2)
    for dp in (0, 1):
        args = make_args(bool(dp))
        npd = normal_pred.clone().requires_grad_(True)
        loss = rmlsp.calc_def_normal_loss(args, {"Normal": npd}, normal_lab.clone(), mask.clone(), [index1, index2], "cpu")
        loss.backward()
        out["normal_loss_dp%d" % dp], out["d_normal_dp%d" % dp] = npy(loss), npy(npd.grad)
        pv, dn = pvec.clone().requires_grad_(True), dens.clone().requires_grad_(True)
        kl, mae = rmlsp.deform_densityloss(args, {"density": pv, "density_mse": dn}, dlab.clone(), dval.clone(), mask.clone(),
                                           [index1, index2], "cpu")
        (kl + mae).backward()
        out["kl_dp%d" % dp], out["mae_dp%d" % dp] = npy(kl), npy(mae)
        out["dkl_density_dp%d" % dp], out["dkl_density_mse_dp%d" % dp] = npy(pv.grad), npy(dn.grad)
    for al in (0, 1):
        args = make_args(False)
        pv = pvec.clone().requires_grad_(True)
        loss = rmlsp.calc_def_density_loss(args, {"density": pv}, dcls.clone(), mask.clone(), [index1, index2], "cpu",
                                           torch.nn.NLLLoss(reduction='none'), all=bool(al))
        loss.backward()
        out["cdl_loss_all%d" % al], out["d_cdl_density_all%d" % al] = npy(loss), npy(pv.grad)
    return out


def main():
    ref_import.install_stubs()
    _, _, rmlsp = ref_import.import_reference()
    import utils.pc_utils as rpc                                           # noqa: E402  (reference, CPU)
    torch.set_num_threads(8)
    for name, args in (("def_losses_s0_B4_N1024.npz", (0, 4, 1024)), ("def_losses_s1_B2_N2048.npz", (1, 2, 2048)),
                       ("def_losses_tie_s2_B2_N256.npz", (2, 2, 256, True))):
        c = case(rmlsp, rpc, *args)
        np.savez_compressed(os.path.join(OUT, name), **c)
        m = c["mask"][:, 0]
        print(name, os.path.getsize(os.path.join(OUT, name)), "masked per cloud", m.sum(1))


if __name__ == "__main__":
    main()
