"""Shim for the supervised step of PointSegDA/trainer.py: its lines 221-233 (criterion, sample_criterion, seg_metrics) become

    from seg_supervision import seg_metrics, SegCrossEntropy
    criterion, sample_criterion = SegCrossEntropy(), SegCrossEntropy(reduction='none')
"""
from mlsp_amd.seg_train import seg_metrics, SegCrossEntropy, seg_step  # noqa: F401
