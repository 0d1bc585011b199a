"""CPU checks of the segmentation-supervision feature (csrc/segsup.hip, mlsp_amd/seg_train.py): the float64 restatement the GPU tests
compare with (tests/segsup_restatement.py) reproduces the recorded torch / sklearn values (tests/golden/segsup_*.npz,
tools/make_golden_segsup.py) and sklearn itself on a grid of cases; the module refuses what is not built; the new symbols are declared on
both sides of the ABI; the trainer's shim module imports."""
import glob
import os
import re
import sys

import numpy as np
import pytest
import torch

import segsup_restatement as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "segsup_*.npz")))
SYMBOLS = ("mlsp_seg_ce_fwd_f32", "mlsp_seg_ce_bwd_f32", "mlsp_seg_metrics_i64", "mlsp_seg_workspace_bytes")


def test_fixtures_exist_and_are_small():
    assert len(FIXTURES) == 3, FIXTURES
    for f in FIXTURES:
        assert os.path.getsize(f) < 100 * 1024, (f, os.path.getsize(f))
        z = np.load(f)
        assert all(z[k].dtype.kind in "fi" for k in z.files), f


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_restatement_equals_golden(path):
    z = np.load(path)
    logits, labels = z["logits"], z["labels"]
    C = logits.shape[2]
    mean = sr.cross_entropy(logits, labels, "mean")
    none = sr.cross_entropy(logits, labels, "none", upstream=z["upstream"])
    assert abs(mean["loss"] - z["loss_mean"]) <= 1e-12 * max(1.0, abs(z["loss_mean"]))
    assert sr.adist(none["loss"], z["loss_none"]) <= 1e-12 * max(1.0, np.abs(z["loss_none"]).max())
    assert sr.adist(mean["grad"], z["grad_mean"]) <= 1e-12
    if "grad_none" in z.files:
        assert sr.adist(none["grad"], z["grad_none"]) <= 1e-12 * np.abs(z["upstream"]).max()
    assert mean["n_valid"] == int((labels != -100).sum())
    preds = logits.argmax(axis=2)
    assert np.array_equal(preds, z["preds"])
    miou, acc = sr.batch_metrics(labels, preds, C)
    assert np.array_equal(miou, z["miou"]) and np.array_equal(acc, z["acc"])           # bit-equal


def test_restatement_is_bit_equal_to_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    n = 0
    for N in sr.GRID_N:
        for C in sr.GRID_C:
            for absent in sr.GRID_ABSENT:
                for seed in range(sr.GRID_SEEDS):
                    y, p = sr.grid_case(N, C, absent, seed)
                    miou, acc = sr.cloud_metrics(y, p, C)
                    want = metrics.jaccard_score(y, p, average="macro")
                    assert miou == want and acc == np.mean(y == p), (N, C, absent, seed, miou, want)
                    n += 1
    assert n == 560


def test_restatement_ignores_out_of_range_labels():
    logits = sr.make_logits("randn3", 2, 9, 5, 3)
    labels = sr.make_labels(2, 9, 5, 3)
    labels[0, 2], labels[1, 0], labels[1, 8] = -100, 5 + 3, -100
    r = sr.cross_entropy(logits, labels, "mean")
    assert r["n_valid"] == 15 and not r["grad"][0, 2].any() and not r["grad"][1, 0].any()
    t = labels.copy()
    t[1, 0] = -100
    want = torch.nn.functional.cross_entropy(torch.from_numpy(logits).double().permute(0, 2, 1), torch.from_numpy(t))
    assert abs(r["loss"] - want.item()) <= 1e-12
    allgone = sr.cross_entropy(logits, np.full_like(labels, -100), "mean")
    assert np.isnan(allgone["loss"]) and not allgone["grad"].any()
    assert all(np.isnan(v) for v in sr.cloud_metrics(np.full(4, -100), np.zeros(4, dtype=np.int64), 5))


def test_module_refuses_what_is_not_built():
    from mlsp_amd.seg_train import SegCrossEntropy
    with pytest.raises(NotImplementedError):
        SegCrossEntropy(weight=torch.ones(8))
    with pytest.raises(NotImplementedError):
        SegCrossEntropy(label_smoothing=0.1)
    assert SegCrossEntropy().reduction == "mean" and SegCrossEntropy(reduction="none").reduction == "none"
    with pytest.raises(TypeError):                             # nn.CrossEntropyLoss has size_average in second place: keywords only after weight
        SegCrossEntropy(None, "none")


def test_no_cpu_fallback():
    from mlsp_amd import _lib, seg_train
    with pytest.raises(_lib.MlspLibraryError):
        seg_train.SegCrossEntropy()(torch.zeros(2, 16, 8).permute(0, 2, 1), torch.zeros(2, 16, dtype=torch.int64))
    with pytest.raises(_lib.MlspLibraryError):
        seg_train.seg_metrics(torch.zeros(2, 16, dtype=torch.int64), torch.zeros(2, 16, dtype=torch.int64))


def test_symbols_are_declared_on_both_sides():
    from mlsp_amd import _lib
    header = open(os.path.join(ROOT, "include", "mlsp_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert "precision" not in re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, header, flags=re.S).group(1), name
    assert _lib.ABI_VERSION == 14
    lib = _lib.load()
    # the shape limits are answered on the host: 0 bytes = refused
    assert lib.mlsp_seg_workspace_bytes(16, 2048, 8) > 0
    assert lib.mlsp_seg_workspace_bytes(1, 1, 65) == 0 and lib.mlsp_seg_workspace_bytes(1, 1, 0) == 0
    assert lib.mlsp_seg_workspace_bytes(0, 1, 8) == 0 and lib.mlsp_seg_workspace_bytes(1 << 16, 1 << 15, 8) == 0
    # refusals launch nothing, so they are reachable without a GPU: MLSP_ERR_UNSUPPORTED = -3
    assert lib.mlsp_seg_ce_fwd_f32(None, 65, None, 1, 1, 65, None, None, None, None, None, None, 0, None) == -3
    assert lib.mlsp_seg_ce_bwd_f32(None, 0, None, None, 1, 1, 0, None, None, None, None, None) == -3
    assert lib.mlsp_seg_metrics_i64(None, None, 1, 1, 65, None, None, 0, None) == -3


def test_shim_module_imports():
    shim = os.path.join(ROOT, "mlsp_amd", "shims", "PointSegDA")
    sys.path.insert(0, shim)
    try:
        sys.modules.pop("seg_supervision", None)
        import seg_supervision
        from mlsp_amd import seg_train
        assert seg_supervision.seg_metrics is seg_train.seg_metrics and seg_supervision.SegCrossEntropy is seg_train.SegCrossEntropy
    finally:
        sys.path.remove(shim)
        sys.modules.pop("seg_supervision", None)
