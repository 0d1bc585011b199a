"""Float64 restatement of the segmentation-supervision kernels (csrc/segsup.hip) and the seeded cases of tests/test_gpu_segsup.py and
tests/test_segsup_cpu.py.  CPU only, numpy and torch.

Cross-entropy: lse = m + log sum exp(x - m) in float64 on the fp32 logits, loss = lse - x[label]; a label outside [0, C) is ignored (no
loss, no gradient, not a valid point); 'mean' divides by the number of valid points (0 / 0 = NaN).  The gradient is written out, not taken
from autograd: (softmax - one-hot) g.

Metrics of one cloud from integer counts over its valid points -- tp[c], true[c], pred[c]:
  mIoU = (sum over the classes with true[c] + pred[c] > 0 of tp[c] / (true[c] + pred[c] - tp[c])) / (number of such classes)
  acc  = correct / valid
each quotient one float64 division.  The sum is written out in the order numpy's add.reduce takes over the quotients in ascending c
(sum_numpy below): left to right below eight values, eight running sums combined pairwise from eight on -- a plain left-to-right sum
differs from sklearn in the last bit once eight classes are present.  That is sklearn.metrics.jaccard_score(average='macro') and
np.mean(y_true == y_pred) bit for bit (tests/test_segsup_cpu.py compares them where sklearn is installed).

Bounds of the GPU tests.  distance = max |got - want64| (absolute), yardstick = the same distance of torch's own fp32 F.cross_entropy on
the CPU, bar = max(floor, 3 yardstick) with floor = 2^-22 max(1, max |lse|) for losses and 2^-22 max |g| for gradient entries (softmax
minus one-hot lies in [-1, 1])."""
import numpy as np
import torch

FLOOR = 2.0 ** -22
METRIC_ULPS = 4


def valid_mask(labels, C):
    labels = np.asarray(labels)
    return (labels >= 0) & (labels < C)


def lse64(logits):
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]


def cross_entropy(logits, labels, reduction="mean", upstream=None):
    """logits [B, N, C] fp32 (values taken as they are, arithmetic in float64), labels [B, N] int64 ->
    dict(loss (scalar or [B, N]), grad [B, N, C], lse [B, N], n_valid, per_point [B, N], cloud_sum [B]); upstream: the incoming gradient,
    a scalar for 'mean' (default 1), [B, N] for 'none' (default ones)"""
    x = np.asarray(logits, dtype=np.float64)
    labels = np.asarray(labels)
    B, N, C = x.shape
    ok = valid_mask(labels, C)
    lse = lse64(x)
    safe = np.where(ok, labels, 0)
    xl = np.take_along_axis(x, safe[..., None], axis=2)[..., 0]
    per_point = np.where(ok, lse - xl, 0.0)
    n_valid = int(ok.sum())
    soft = np.exp(x - lse[..., None])
    onehot = np.zeros_like(x)
    np.put_along_axis(onehot, safe[..., None], 1.0, axis=2)
    if reduction == "mean":
        with np.errstate(invalid="ignore", divide="ignore"):
            loss = np.float64(per_point.sum()) / np.float64(n_valid)
            g = np.full((B, N), (1.0 if upstream is None else float(upstream))) / np.float64(n_valid)
    else:
        loss = per_point
        g = np.ones((B, N)) if upstream is None else np.asarray(upstream, dtype=np.float64)
    grad = np.where(ok[..., None], (soft - onehot) * g[..., None], 0.0)
    return dict(loss=loss, grad=grad, lse=lse, n_valid=n_valid, per_point=per_point, cloud_sum=per_point.sum(axis=1), g=g)


def counts(labels, preds, C):
    """integer counts of one cloud over its valid points -> (tp [C], true [C], pred [C], correct, valid); a prediction outside [0, C)
    counts for no predicted class"""
    labels, preds = np.asarray(labels).reshape(-1), np.asarray(preds).reshape(-1)
    ok = valid_mask(labels, C)
    y, p = labels[ok], preds[ok]
    tp = np.bincount(y[y == p], minlength=C).astype(np.int64)
    tr = np.bincount(y, minlength=C).astype(np.int64)
    inside = (p >= 0) & (p < C)
    pr = np.bincount(p[inside], minlength=C).astype(np.int64)
    return tp, tr, pr, int((y == p).sum()), int(ok.sum())


def sum_numpy(a):
    """the float64 sum of at most 128 values in the order of numpy's add.reduce, written out with scalar additions"""
    a = [np.float64(v) for v in a]
    n = len(a)
    assert n <= 128
    if n < 8:
        s = np.float64(0.0)
        for v in a:
            s = s + v
        return s
    r = a[:8]
    i = 8
    while i < n - n % 8:
        r = [r[j] + a[i + j] for j in range(8)]
        i += 8
    s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        s = s + v
    return s


def cloud_metrics(labels, preds, C):
    """(mIoU, acc) of one cloud, float64, in the order stated in the module docstring"""
    tp, tr, pr, correct, valid = counts(labels, preds, C)
    ious = [np.float64(tp[c]) / np.float64(tr[c] + pr[c] - tp[c]) for c in range(C) if tr[c] + pr[c] > 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return sum_numpy(ious) / np.float64(len(ious)), np.float64(correct) / np.float64(valid)


def batch_metrics(labels, preds, C):
    """-> (miou [B], acc [B]) float64"""
    rows = [cloud_metrics(labels[b], preds[b], C) for b in range(len(labels))]
    return np.array([r[0] for r in rows], dtype=np.float64), np.array([r[1] for r in rows], dtype=np.float64)


def trainer_metrics(labels, preds, C):
    """the trainer's seg_metrics: Python sums over the batch, ascending cloud order"""
    miou, acc = batch_metrics(labels, preds, C)
    m = a = 0
    for b in range(len(miou)):
        m += float(miou[b])
        a += float(acc[b])
    return m, a


def ulps(a, b):
    """largest distance of two float64 arrays in units in the last place (NaN equals NaN)"""
    a, b = np.atleast_1d(np.asarray(a, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    both_nan = np.isnan(a) & np.isnan(b)
    if (np.isnan(a) != np.isnan(b)).any():
        return np.inf
    a, b = np.where(both_nan, 0.0, a), np.where(both_nan, 0.0, b)
    d = np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return float(d.max()) if d.size else 0.0


# --------------------------------------------------------------------------------------------- yardstick and bars
def torch_fp32(logits, labels, reduction="mean", upstream=None):
    """torch's own fp32 F.cross_entropy on the CPU, the trainer's call shape (the permuted view), with its autograd gradient ->
    dict(loss, grad).  Labels must be valid or -100."""
    x = torch.as_tensor(np.asarray(logits)).clone().requires_grad_(True)
    y = torch.as_tensor(np.asarray(labels))
    loss = torch.nn.functional.cross_entropy(x.permute(0, 2, 1), y, reduction=reduction)
    if reduction == "mean":
        loss.backward(None if upstream is None else torch.tensor(float(upstream)))
    else:
        loss.backward(torch.ones_like(loss) if upstream is None else torch.as_tensor(np.asarray(upstream, dtype=np.float32)))
    return dict(loss=loss.detach().numpy().astype(np.float64), grad=x.grad.numpy().astype(np.float64))


def adist(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0


def loss_bar(want, yard):
    """bar of a loss (per point or mean) given the float64 result dict and torch's fp32 distance"""
    return max(FLOOR * max(1.0, float(np.abs(want["lse"]).max())), 3 * yard)


def grad_bar(want, yard):
    return max(FLOOR * float(np.abs(want["g"]).max()), 3 * yard)


# --------------------------------------------------------------------------------------------- seeded cases
KINDS = ("randn3", "shift1e4", "spread80", "ties")


def make_logits(kind, B, N, C, seed):
    rs = np.random.RandomState(seed)
    if kind == "randn3":
        x = 3.0 * rs.randn(B, N, C)
    elif kind == "shift1e4":
        x = 3.0 * rs.randn(B, N, C) + 1e4
    elif kind == "spread80":
        x = rs.uniform(-80.0, 80.0, (B, N, C))
    elif kind == "ties":                                    # quantised to {-1, 0, 1}: every row has repeated maxima once C > 3
        x = rs.randint(-1, 2, (B, N, C)).astype(np.float64)
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


def make_labels(B, N, C, seed, absent=()):
    """int64 [B, N] uniform over the classes not in `absent`"""
    rs = np.random.RandomState(seed + 7919)
    classes = np.array([c for c in range(C) if c not in absent] or [0], dtype=np.int64)
    return classes[rs.randint(0, len(classes), (B, N))]


# the sklearn comparison grid of tests/test_segsup_cpu.py: 7 x 4 x 4 x 5 = 560 cases
GRID_N = (1, 2, 7, 255, 256, 257, 2048)
GRID_C = (2, 8, 10, 13)
GRID_ABSENT = ("none", "labels", "preds", "both")
GRID_SEEDS = 5


def grid_case(N, C, absent, seed):
    """(labels [N], preds [N]) with one class missing from the labels, the predictions, or both"""
    rs = np.random.RandomState(1000 * seed + 10 * N + C)
    gone = rs.randint(0, C)
    def draw(skip):
        classes = np.array([c for c in range(C) if not (skip and c == gone)] or [0])
        return classes[rs.randint(0, len(classes), N)].astype(np.int64)
    return draw(absent in ("labels", "both")), draw(absent in ("preds", "both"))
