"""Drop-in for PointDA/hengshuang_transformer/transformer.py (the vector-attention TransformerBlock) backed by the MI355X kernels."""
from mlsp_amd.transformer import TransformerBlock  # noqa: F401
