"""Generate tests/golden/segsup_*.npz: what the segmentation trainer's supervised step computes (PointSegDA/trainer.py:221-233, 253-258),
taken from the libraries it calls, on the CPU in float64:

  torch's nn.CrossEntropyLoss on logits.permute(0, 2, 1), reductions 'mean' and 'none', with the autograd gradient of each
    ('none' under a recorded random upstream gradient);
  preds = torch's arg-max over the classes of the fp32 logits;
  per cloud sklearn.metrics.jaccard_score(y_true, y_pred, average='macro') and np.mean(y_true == y_pred) -- on the points whose label is
    not -100 where a fixture has ignored labels.

Numeric arrays only.  Needs scikit-learn; the tests that read the fixtures do not.

    python tools/make_golden_segsup.py
"""
import os

import numpy as np
import torch
from sklearn.metrics import jaccard_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")

# name -> (B, N, C, scale, classes absent from the labels, fraction of -100 labels, reductions whose gradient is recorded); the float64
# gradients are the bulk of a file, so the largest shape records one of the two
FIXTURES = {
    "segsup_c8": (3, 257, 8, 3.0, (), 0.0, ("mean",)),
    "segsup_c13": (2, 130, 13, 5.0, (4, 11), 0.0, ("mean", "none")),
    "segsup_ignore": (2, 129, 10, 3.0, (), 0.1, ("mean", "none")),
}


def make(name, B, N, C, scale, absent, p_ignore, grads):
    rs = np.random.RandomState(sum(map(ord, name)))
    logits = (scale * rs.randn(B, N, C)).astype(np.float32)
    logits[:, :, list(absent)] -= 50.0                      # never predicted either: absent from labels and predictions
    classes = np.array([c for c in range(C) if c not in absent], dtype=np.int64)
    labels = classes[rs.randint(0, len(classes), (B, N))]
    right = rs.uniform(size=(B, N)) < 0.5                   # half of the points are predicted right
    labels[right] = logits.argmax(axis=2)[right]
    labels[rs.uniform(size=(B, N)) < p_ignore] = -100
    upstream = rs.randn(B, N).astype(np.float32)
    out = dict(logits=logits, labels=labels, upstream=upstream)
    y = torch.from_numpy(labels)
    for reduction in ("mean", "none"):
        x = torch.from_numpy(logits).double().requires_grad_(True)
        loss = torch.nn.CrossEntropyLoss(reduction=reduction)(x.permute(0, 2, 1), y)
        if reduction == "mean":
            loss.backward()
        else:
            loss.backward(torch.from_numpy(upstream).double())
        out["loss_" + reduction] = loss.detach().numpy()
        if reduction in grads:
            out["grad_" + reduction] = x.grad.numpy()
    preds = torch.from_numpy(logits).argmax(dim=2).numpy()
    out["preds"] = preds
    miou, acc = [], []
    for b in range(B):
        keep = labels[b] != -100
        want, got = labels[b][keep], preds[b][keep]
        miou.append(jaccard_score(want, got, average="macro"))
        acc.append((want == got).mean())
    out["miou"], out["acc"] = np.array(miou, dtype=np.float64), np.array(acc, dtype=np.float64)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, loss %.6f, miou %s" % (path, os.path.getsize(path), out["loss_mean"], out["miou"]))


if __name__ == "__main__":
    for name, spec in FIXTURES.items():
        make(name, *spec)
