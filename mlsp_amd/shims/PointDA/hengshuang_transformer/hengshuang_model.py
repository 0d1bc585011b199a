"""Drop-in for PointDA/hengshuang_transformer/hengshuang_model.py (the Point Transformer models) backed by the MI355X kernels."""
from mlsp_amd.hengshuang_model import (Backbone, PointTransformerCls, PointTransformerDef, PointTransformerSeg,  # noqa: F401
                                       TransitionDown, TransitionUp)
