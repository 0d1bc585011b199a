"""The supervised half of a PointSegDA training step on the device (PointSegDA/trainer.py:221-233, 253-258, 309-319): the trainer's
`criterion` / `sample_criterion`, its `seg_metrics`, and the three together from one pass over the logits (csrc/segsup.hip).
No CPU fallback; nothing here copies to the host except the result rows of `seg_metrics`, which the trainer adds to Python floats.
"""
from torch import nn

from . import functional as Fh


class SegCrossEntropy(nn.Module):
    """Stands where the trainer's `nn.CrossEntropyLoss()` and `nn.CrossEntropyLoss(reduction='none')` stand.

    forward(input, target) takes what the trainer passes -- `logits['seg'].permute(0, 2, 1)`, the [B, C, N] view of the head's [B, N, C]
    output, with labels [B, N] -- and reads the logits in place: strides (N C, 1, C) are recognised and nothing is copied.  Plain [R, C]
    logits with [R] labels are one cloud of R points.  Any other [B, C, N] layout costs one contiguous copy of the un-permuted form.
    The gradient comes back through the view, in the layout of the tensor the view was taken from.

    Labels equal to ignore_index (-100 only, torch's default) are left out of the loss and the mean's denominator and get no gradient;
    so is every other label outside [0, C), where torch raises.  C <= 64.  weight= and label_smoothing are not built.  Everything after
    `weight` is keyword-only: nn.CrossEntropyLoss has other positionals there (size_average, ignore_index, reduce)."""

    def __init__(self, weight=None, *, reduction="mean", ignore_index=-100, label_smoothing=0.0):
        super().__init__()
        if weight is not None:
            raise NotImplementedError("SegCrossEntropy: class weights are not built")
        if label_smoothing != 0:
            raise NotImplementedError("SegCrossEntropy: label smoothing is not built")
        if reduction not in ("mean", "none"):
            raise NotImplementedError("SegCrossEntropy: reduction=%r (the trainer uses 'mean' and 'none')" % (reduction,))
        if ignore_index != -100:
            raise NotImplementedError("SegCrossEntropy: ignore_index=%r (every label outside [0, C) is ignored; only the default is accepted)"
                                      % (ignore_index,))
        self.reduction, self.ignore_index = reduction, ignore_index

    def forward(self, input, target):
        if input.dim() == 2:                                     # [R, C], [R]
            loss = Fh.seg_cross_entropy(input.unsqueeze(0), target.unsqueeze(0), self.reduction)
            return loss if self.reduction == "mean" else loss[0]
        if input.dim() != 3:
            raise ValueError("SegCrossEntropy: input %s (expected [B, C, N] or [R, C])" % (tuple(input.shape),))
        return Fh.seg_cross_entropy(input.permute(0, 2, 1), target, self.reduction)     # the trainer's view, un-permuted: no copy


def seg_step(logits, labels):
    """(loss, preds, miou, acc) of one supervised step from logits [B, N, C] and labels [B, N], one pass over the logits: the mean
    cross-entropy (with its gradient), preds = logits.max(dim=2)[1], and per cloud [B] float64 mIoU and accuracy, all on the device."""
    loss, preds, miou, acc, _ = Fh.seg_cross_entropy(logits, labels, "mean", with_metrics=True)
    return loss, preds, miou, acc


def seg_metrics(labels, preds, num_classes=64):
    """The trainer's seg_metrics(labels, preds) -> (mIOU, accuracy): the SUMS over the batch of every cloud's
    jaccard_score(average='macro') and np.mean(labels == preds), as Python floats added in ascending cloud order.  One launch pair and one
    copy of the [B + 1, 5] float64 result rows to the host instead of 2 B copies and B sklearn calls.  Class ids lie in
    [0, num_classes), num_classes <= 64: a label outside is left out of the counts (sklearn would count it), so a caller with fewer than
    64 classes need not say so, one with more cannot use this."""
    rows = Fh._seg_metrics_stats(labels.detach().long(), preds.detach().long(), int(num_classes)).cpu()[:-1, 1:3].tolist()
    m = a = 0.0
    for iou, acc in rows:
        m += iou
        a += acc
    return m, a
