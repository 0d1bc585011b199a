"""Every launch the GEMM tests make through functional.gemm (mlsp_gemm_f32), each with the kernel it reaches: one table, like knn_shapes.py.

A row is R(mode, ta, tb, M, N, K, label, via=, reduce=, pad=, off=, bias=):
  mode    the product mode of the call ("fp32", "bf16", "bf16x6", "f16x3");
  label   what tools/gemm_plan_host_check prints for the plan (csrc/gemm_plan.h) of that launch:
          FAMILY/bm/ns=<n>/xcd=<m>[/fast][/pieces | /pieces:six][/thin?][/skinny?], FOLD64:<label of the 128 x 128 x K/2 launch it runs>.
          pieces: mode f16x3 on the split kernel, where the launcher measures both operands and runs the two-piece f16 products;
          pieces:six: eligible, but measuring does not pay (gemm_pieces_measure_pays), so the launch stays on the six bf16 products --
          such a row tests bf16x6 a second time;  thin? / skinny?: thin.hip / skinny.hip are offered the launch first;
  via     who really runs it: "tile" (the kernel the label names), "fold" (that kernel at 128 x 128 x K/2, then the 64 x 64 sum), "thin" /
          "skinny" (the offer was taken: no tile kernel is launched; read from thin.hip / skinny.hip, asserted on the GPU);
  reduce  the kernel that sums the slabs of a split-K tile launch (gemm_pick_reduce): VEC8 / VEC4 / VEC1 / WAVE / SCALAR, "-": one pass;
  pad     floats added to the pitches of (A, B, C) over their row lengths (C through out=; a pitch that is no multiple of 4 takes the
          scalar loads of the bounds-checked kernel);  off: floats (4 bytes each) by which A / B start off a 16-byte boundary;
  bias    0 none, 1 on a 16-byte boundary, 2 a [1:] view, 4 bytes off one.

tests/test_gemm_plan_cpu.py asserts every label and reducer against the plan and that the rows cover every label the tool's sweep reaches
for plain and bias launches (the number of splits apart), all five reducers and every layout of every family;
tests/test_gpu_gemm_variants.py launches every row and asserts that the kernel that ran is the one named, with exact results;
tests/test_gpu_kernels.py takes the shapes of its GEMM tests from TESTS.

Not covered: the launch options stat, sel, xf, grp, bs, dy, accumulate and gbias (and the UNFOLD reducers behind unfold_dw) cannot be
reached through mlsp_gemm_f32; they stay with the layer tests.

Mode f16x3, which rows run the f16 pieces: every row labelled /pieces -- 128- and 64-row tiles in one pass with and without an XCD map,
split-K at xcd_map 0, 1, 2 and 3; all four layouts at both tile heights, under split-K, and at xcd_map 0.  Every pieces label the tool's
sweep meets is pinned and run (products up to 2^34 + 2^32, the largest the tests launch; the sweep takes every panel count below 16,
where xcd_map and the tile height turn, against wide N).  Rows labelled /pieces:six say so: they are on the six bf16 products."""
from collections import namedtuple

Row = namedtuple("Row", "mode ta tb M N K label via reduce pad off bias")
FAMILIES = ("FOLD64", "N64", "F32_EDGE", "F32", "BF16", "SPLIT")                    # GemmFamily
REDUCERS = ("VEC8", "VEC4", "VEC1", "WAVE", "SCALAR", "UNFOLD8", "UNFOLD4", "UNFOLD1")      # GemmReduce
MODES = {"fp32": 0, "bf16": 1, "bf16x6": 2, "f16x3": 3}


def R(mode, ta, tb, M, N, K, label, via="tile", reduce="-", pad=(0, 0, 0), off=(0, 0), bias=0):
    return Row(mode, ta, tb, M, N, K, label, via, reduce, pad, off, bias)


# the GEMM tests of tests/test_gpu_kernels.py: test -> every launch it makes
TESTS = {
    "test_gemm": [
        R("f16x3", 0, 1, 300, 200, 64, "F32_EDGE/64/ns=1/xcd=0/thin?"),
        R("f16x3", 0, 1, 1024, 128, 3, "F32_EDGE/64/ns=1/xcd=0/thin?", via="thin"),
        R("f16x3", 0, 0, 257, 130, 100, "F32_EDGE/128/ns=2/xcd=0/thin?", reduce="SCALAR"),
        R("f16x3", 1, 0, 64, 6, 5000, "F32_EDGE/128/ns=53/xcd=0/thin?", via="thin"),
        R("f16x3", 1, 0, 256, 512, 4096, "F32/128/ns=64/xcd=0/fast/thin?", reduce="VEC8"),
        R("f16x3", 0, 1, 32, 512, 1024, "F32_EDGE/128/ns=16/xcd=0/thin?/skinny?", via="skinny"),
        R("f16x3", 0, 1, 4096, 2048, 512, "SPLIT/128/ns=1/xcd=1/fast/pieces/thin?"),
        R("f16x3", 1, 1, 100, 70, 50, "F32_EDGE/128/ns=1/xcd=0/thin?"),
        R("f16x3", 0, 1, 5, 9, 256, "F32_EDGE/128/ns=4/xcd=0/thin?/skinny?", via="skinny"),
        # skinny.hip: <= 32 rows (fwd / dgrad) and 32-deep wgrads, ragged edges
        R("f16x3", 0, 1, 32, 256, 1024, "F32_EDGE/128/ns=16/xcd=0/thin?/skinny?", via="skinny"),
        R("f16x3", 0, 1, 17, 33, 100, "F32_EDGE/128/ns=2/xcd=0/thin?/skinny?", via="skinny"),
        R("f16x3", 0, 0, 32, 1024, 256, "F32_EDGE/128/ns=4/xcd=0/thin?/skinny?", via="skinny"),
        R("f16x3", 0, 0, 7, 50, 9, "F32_EDGE/128/ns=1/xcd=0/thin?/skinny?", via="skinny"),
        R("f16x3", 1, 0, 256, 1024, 32, "F32/64/ns=1/xcd=0/fast/thin?/skinny?", via="skinny"),
        R("f16x3", 1, 0, 9, 256, 20, "F32_EDGE/128/ns=1/xcd=0/thin?/skinny?", via="skinny"),
        R("f16x3", 1, 0, 70, 33, 3, "F32_EDGE/128/ns=1/xcd=0/thin?/skinny?", via="skinny"),
    ],
    # each shape in mode "bf16", then again in the default mode
    "test_gemm_bf16_operand_mode": [
        R("bf16", 0, 1, 1024, 256, 512, "BF16/128/ns=8/xcd=0/fast/thin?", reduce="VEC4"),
        R("f16x3", 0, 1, 1024, 256, 512, "F32/128/ns=8/xcd=0/fast/thin?", reduce="VEC4"),
        R("bf16", 0, 0, 512, 384, 256, "BF16/128/ns=4/xcd=0/fast/thin?", reduce="VEC1"),
        R("f16x3", 0, 0, 512, 384, 256, "F32/128/ns=4/xcd=0/fast/thin?", reduce="VEC1"),
        R("bf16", 1, 0, 256, 128, 8192, "BF16/128/ns=128/xcd=0/fast/thin?", reduce="VEC8"),
        R("f16x3", 1, 0, 256, 128, 8192, "F32/128/ns=128/xcd=0/fast/thin?", reduce="VEC8"),
        R("bf16", 0, 1, 4096, 128, 64, "BF16/64/ns=1/xcd=0/fast/thin?"),
        R("f16x3", 0, 1, 4096, 128, 64, "F32/64/ns=1/xcd=0/fast/thin?"),
        R("bf16", 1, 1, 256, 256, 128, "BF16/128/ns=2/xcd=0/fast/thin?", reduce="VEC1"),
        R("f16x3", 1, 1, 256, 256, 128, "F32/128/ns=2/xcd=0/fast/thin?", reduce="VEC1"),
        R("bf16", 0, 1, 300, 200, 64, "F32_EDGE/64/ns=1/xcd=0/thin?"),                   # off the fast path: the fp32 kernel
        R("f16x3", 0, 1, 300, 200, 64, "F32_EDGE/64/ns=1/xcd=0/thin?"),
    ],
    "test_thin_gemms": [
        R("f16x3", 0, 1, 4096, 128, 3, "F32_EDGE/64/ns=1/xcd=0/thin?", via="thin"),
        R("f16x3", 0, 0, 4096, 128, 3, "F32_EDGE/64/ns=1/xcd=0/thin?", via="thin"),
        R("f16x3", 0, 0, 2048, 256, 16, "F32_EDGE/64/ns=1/xcd=1/thin?", via="thin"),
        R("f16x3", 0, 1, 4096, 3, 128, "F32_EDGE/128/ns=2/xcd=0/thin?", via="thin"),
        R("f16x3", 0, 1, 4096, 16, 256, "F32_EDGE/128/ns=4/xcd=0/thin?", via="thin", bias=1),
        R("f16x3", 0, 0, 4096, 3, 128, "F32_EDGE/128/ns=2/xcd=0/thin?", via="thin"),
        R("f16x3", 1, 0, 3, 128, 4096, "F32_EDGE/128/ns=64/xcd=0/thin?", via="thin"),
        R("f16x3", 1, 0, 16, 256, 8192, "F32_EDGE/128/ns=128/xcd=0/thin?", via="thin"),
        R("f16x3", 1, 0, 128, 3, 4096, "F32_EDGE/128/ns=64/xcd=0/thin?", via="thin"),
        R("f16x3", 1, 0, 256, 16, 2048, "F32_EDGE/128/ns=32/xcd=0/thin?", via="thin"),
        R("f16x3", 1, 0, 64, 3, 8192, "F32_EDGE/128/ns=128/xcd=0/thin?", via="thin"),
        R("f16x3", 1, 0, 3, 64, 8192, "F32_EDGE/128/ns=128/xcd=0/thin?", via="thin"),
        R("f16x3", 0, 1, 32768, 128, 3, "F32_EDGE/64/ns=1/xcd=0/thin?", via="thin", bias=1),
        R("f16x3", 1, 0, 3, 128, 32768, "F32_EDGE/128/ns=256/xcd=0/thin?", via="thin"),
    ],
    "test_gemm_matches_fma_chain_bitwise": [
        R("f16x3", 0, 1, 64, 40, 24, "F32_EDGE/128/ns=1/xcd=0/thin?"),
    ],
    # each shape in modes "fp32" (the yardstick), "bf16x6" and "f16x3".  Both tile heights, split-K, all four layouts; of the f16x3 cases,
    # (32768, 256, 512), (512, 256, 32768), (4096, 1024, 128) and (256, 256, 16384) stay on the six bf16 products
    "test_gemm_split_bf16_accuracy": [
        R("fp32", 0, 1, 32768, 256, 512, "F32/64/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 1, 32768, 256, 512, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
        R("f16x3", 0, 1, 32768, 256, 512, "SPLIT/128/ns=1/xcd=1/fast/pieces:six/thin?"),
        R("fp32", 0, 0, 32768, 512, 256, "F32/64/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 0, 32768, 512, 256, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
        R("f16x3", 0, 0, 32768, 512, 256, "SPLIT/128/ns=1/xcd=1/fast/pieces/thin?"),
        R("fp32", 1, 0, 512, 256, 32768, "F32/128/ns=64/xcd=0/fast/thin?", reduce="VEC8"),
        R("bf16x6", 1, 0, 512, 256, 32768, "SPLIT/128/ns=64/xcd=3/fast/thin?", reduce="VEC8"),
        R("f16x3", 1, 0, 512, 256, 32768, "SPLIT/128/ns=64/xcd=3/fast/pieces:six/thin?", reduce="VEC8"),
        R("fp32", 0, 1, 4096, 1024, 128, "F32/64/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 1, 4096, 1024, 128, "SPLIT/64/ns=1/xcd=1/fast/thin?"),
        R("f16x3", 0, 1, 4096, 1024, 128, "SPLIT/64/ns=1/xcd=1/fast/pieces:six/thin?"),
        R("fp32", 0, 1, 32768, 1024, 512, "F32/128/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 1, 32768, 1024, 512, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
        R("f16x3", 0, 1, 32768, 1024, 512, "SPLIT/128/ns=1/xcd=1/fast/pieces/thin?"),
        R("fp32", 0, 0, 65536, 1024, 128, "F32/128/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 0, 65536, 1024, 128, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
        R("f16x3", 0, 0, 65536, 1024, 128, "SPLIT/128/ns=1/xcd=1/fast/pieces/thin?"),
        R("fp32", 1, 1, 256, 256, 16384, "F32/128/ns=128/xcd=0/fast/thin?", reduce="VEC8"),
        R("bf16x6", 1, 1, 256, 256, 16384, "SPLIT/128/ns=128/xcd=3/fast/thin?", reduce="VEC8"),
        R("f16x3", 1, 1, 256, 256, 16384, "SPLIT/128/ns=128/xcd=3/fast/pieces:six/thin?", reduce="VEC8"),
        R("fp32", 1, 0, 1024, 512, 32768, "F32/128/ns=16/xcd=0/fast/thin?", reduce="VEC4"),
        R("bf16x6", 1, 0, 1024, 512, 32768, "SPLIT/128/ns=16/xcd=3/fast/thin?", reduce="VEC4"),
        R("f16x3", 1, 0, 1024, 512, 32768, "SPLIT/128/ns=16/xcd=3/fast/pieces/thin?", reduce="VEC4"),
        # a k-major / row-major A operand on the 64-row tile (256-511 tiles of 128 rows, no split-K)
        R("fp32", 1, 0, 2048, 2048, 512, "F32/64/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 1, 0, 2048, 2048, 512, "SPLIT/64/ns=1/xcd=1/fast/thin?"),
        R("f16x3", 1, 0, 2048, 2048, 512, "SPLIT/64/ns=1/xcd=1/fast/pieces/thin?"),
        R("fp32", 1, 1, 2048, 2560, 256, "F32/64/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 1, 1, 2048, 2560, 256, "SPLIT/64/ns=1/xcd=1/fast/thin?"),
        R("f16x3", 1, 1, 2048, 2560, 256, "SPLIT/64/ns=1/xcd=1/fast/pieces/thin?"),
        R("fp32", 0, 0, 2048, 2048, 512, "F32/64/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 0, 2048, 2048, 512, "SPLIT/64/ns=1/xcd=1/fast/thin?"),
        R("f16x3", 0, 0, 2048, 2048, 512, "SPLIT/64/ns=1/xcd=1/fast/pieces/thin?"),
    ],
    # each shape in modes "fp32" and "bf16x6": the same kernel (K = 128 at 4096 rows splits K in two)
    "test_gemm_split_short_k_stays_on_fp32_kernel": [
        R("fp32", 0, 1, 16384, 128, 64, "F32/64/ns=1/xcd=0/fast/thin?"),
        R("bf16x6", 0, 1, 16384, 128, 64, "F32/64/ns=1/xcd=0/fast/thin?"),
        R("fp32", 0, 1, 4096, 128, 128, "F32/128/ns=2/xcd=0/fast/thin?", reduce="VEC1"),
        R("bf16x6", 0, 1, 4096, 128, 128, "F32/128/ns=2/xcd=0/fast/thin?", reduce="VEC1"),
        R("fp32", 0, 1, 1024, 512, 96, "F32/64/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 1, 1024, 512, 96, "F32/64/ns=1/xcd=1/fast/thin?"),
    ],
    "test_precision_is_per_call_two_threads_and_late_backward": [
        R("fp32", 0, 1, 32768, 256, 256, "F32/64/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 1, 32768, 256, 256, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
    ],
    # the folded launches in modes "fp32" and "bf16x6" (the 128 x 128 x K/2 product inside: two K tiles per split do not pay for the split
    # kernel until K = 524288), then the neighbour at pitch 96 in the default mode
    "test_gemm_fold64_weight_gradient": [
        R("fp32", 1, 0, 64, 64, 8192, "FOLD64:F32/128/ns=64/xcd=0/fast/thin?", via="fold", reduce="VEC8"),
        R("bf16x6", 1, 0, 64, 64, 8192, "FOLD64:F32/128/ns=64/xcd=0/fast/thin?", via="fold", reduce="VEC8"),
        R("fp32", 1, 0, 64, 64, 65536, "FOLD64:F32/128/ns=256/xcd=0/fast/thin?", via="fold", reduce="VEC8"),
        R("bf16x6", 1, 0, 64, 64, 65536, "FOLD64:F32/128/ns=256/xcd=0/fast/thin?", via="fold", reduce="VEC8"),
        R("fp32", 1, 0, 64, 64, 524288, "FOLD64:F32/128/ns=256/xcd=0/fast/thin?", via="fold", reduce="VEC8"),
        R("bf16x6", 1, 0, 64, 64, 524288, "FOLD64:SPLIT/128/ns=256/xcd=0/fast/thin?", via="fold", reduce="VEC8"),
        R("f16x3", 1, 0, 64, 64, 8192, "F32_EDGE/128/ns=128/xcd=0/thin?", reduce="VEC8", pad=(32, 0, 0)),
    ],
    "test_gemm_split_layouts_agree_and_are_linear": [
        R("bf16x6", 0, 1, 32768, 512, 1024, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 0, 0, 32768, 512, 1024, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 1, 1, 32768, 512, 1024, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
        R("bf16x6", 1, 0, 32768, 512, 1024, "SPLIT/128/ns=1/xcd=1/fast/thin?"),
    ],
}

# tests/test_gpu_gemm_variants.py only: the smallest shapes the tool finds for what the tests above leave out
_F32_LIKE = [   # (ta, tb, M, N, K, label behind the family, keywords): the interior-tile kernels, in mode "fp32" (F32) and "bf16" (BF16)
    (0, 0, 128, 128, 32, "128/ns=1/xcd=0/fast/thin?", {}),
    (1, 0, 128, 128, 32, "128/ns=1/xcd=0/fast/thin?/skinny?", dict(bias=1)),                        # (skinny.hip takes no bias in this layout)
    (0, 1, 16384, 1536, 32, "128/ns=1/xcd=1/fast/thin?", {}),                                        # 1536 tiles of 128 rows: the fewest that keep them
    (1, 0, 16384, 1536, 32, "128/ns=1/xcd=1/fast/thin?/skinny?", dict(pad=(4, 4, 4), bias=2)),
    (1, 1, 128, 128, 128, "128/ns=2/xcd=0/fast/thin?", dict(reduce="VEC1")),
    (0, 0, 384, 256, 2048, "128/ns=32/xcd=0/fast/thin?", dict(reduce="WAVE", pad=(4, 4, 4), bias=1)),   # a pitched C: no vector reduce
    (0, 1, 2048, 256, 128, "128/ns=2/xcd=1/fast/thin?", dict(reduce="VEC1", bias=1)),
    (1, 1, 2048, 256, 128, "128/ns=2/xcd=1/fast/thin?", dict(reduce="SCALAR", pad=(4, 4, 0), bias=2)),  # the bias view alone: scalar reduce
    (1, 0, 256, 128, 64, "64/ns=1/xcd=0/fast/thin?", {}),
    (1, 0, 256, 128, 32, "64/ns=1/xcd=0/fast/thin?/skinny?", dict(pad=(4, 4, 4), bias=1)),
    (0, 0, 1024, 256, 64, "64/ns=1/xcd=1/fast/thin?", dict(pad=(0, 4, 4))),
    (1, 1, 1024, 256, 96, "64/ns=1/xcd=1/fast/thin?", dict(pad=(4, 0, 0), bias=2)),
    (1, 0, 1024, 256, 32, "64/ns=1/xcd=1/fast/thin?/skinny?", dict(bias=1)),
]
_SPLIT = [      # the split kernel, in mode "bf16x6" and "f16x3": (ta, tb, M, N, K, label, ":six" where f16x3 stays on six products, keywords)
    (0, 0, 65536, 128, 128, "128/ns=1/xcd=0/fast", ":six", {}),
    (0, 1, 4096, 2048, 128, "128/ns=1/xcd=1/fast", "", {}),                                      # 128-row tiles, each layout
    (0, 0, 4096, 2048, 128, "128/ns=1/xcd=1/fast", "", dict(pad=(4, 4, 4), bias=1)),
    (1, 0, 4096, 2048, 128, "128/ns=1/xcd=1/fast", "", {}),
    (1, 1, 4096, 2048, 128, "128/ns=1/xcd=1/fast", "", dict(pad=(4, 4, 0), bias=2)),
    (0, 0, 16384, 512, 128, "128/ns=1/xcd=1/fast", ":six", {}),
    (0, 1, 1920, 4608, 128, "128/ns=1/xcd=0/fast", "", {}),                  # 15 panels of 128 rows x 36 column tiles: no XCD map, each layout
    (0, 0, 1920, 4608, 128, "128/ns=1/xcd=0/fast", "", dict(pad=(4, 4, 4), bias=1)),
    (1, 0, 1920, 4608, 128, "128/ns=1/xcd=0/fast", "", dict(bias=2)),
    (1, 1, 1920, 4608, 128, "128/ns=1/xcd=0/fast", "", dict(pad=(4, 4, 0))),
    (0, 0, 1408, 2048, 512, "128/ns=3/xcd=0/fast", "", dict(reduce="VEC1")),       # split-K without an XCD map (splits no multiple of 8), each layout
    (1, 0, 1408, 1664, 512, "128/ns=4/xcd=0/fast", "", dict(reduce="SCALAR", bias=2)),
    (0, 1, 1664, 1024, 1024, "128/ns=5/xcd=0/fast", "", dict(reduce="VEC1", pad=(4, 4, 0))),
    (1, 1, 896, 1664, 1024, "128/ns=6/xcd=0/fast", "", dict(reduce="VEC1", bias=1)),
    (0, 1, 16384, 128, 512, "128/ns=4/xcd=0/fast", ":six", dict(reduce="VEC1")),
    (1, 0, 16384, 128, 512, "128/ns=4/xcd=0/fast", ":six", dict(reduce="SCALAR", pad=(4, 4, 4), bias=1)),
    (0, 0, 2048, 256, 2048, "128/ns=16/xcd=1/fast", ":six", dict(reduce="VEC4")),
    (0, 1, 2048, 1024, 1024, "128/ns=4/xcd=1/fast", "", dict(reduce="VEC1", bias=1)),
    (0, 0, 128, 512, 16384, "128/ns=128/xcd=2/fast", ":six", dict(reduce="VEC8", bias=1)),
    (1, 0, 1024, 2048, 1024, "128/ns=4/xcd=2/fast", "", dict(reduce="VEC1", pad=(4, 4, 0))),
    (0, 1, 1024, 2048, 1024, "128/ns=4/xcd=2/fast", "", dict(reduce="VEC1", bias=1)),
    (1, 0, 1024, 1024, 1024, "128/ns=8/xcd=3/fast", ":six", dict(reduce="VEC4")),
    (0, 0, 1024, 1024, 2048, "128/ns=8/xcd=3/fast", "", dict(reduce="SCALAR", bias=2)),          # split-K, each layout
    (1, 0, 1024, 1024, 2048, "128/ns=8/xcd=3/fast", "", dict(reduce="SCALAR", pad=(4, 4, 4))),
    (0, 1, 1024, 1024, 2048, "128/ns=8/xcd=3/fast", "", dict(reduce="VEC4")),
    (1, 1, 1024, 1024, 2048, "128/ns=8/xcd=3/fast", "", dict(reduce="VEC4", bias=1)),
    (0, 1, 32768, 128, 128, "64/ns=1/xcd=0/fast", ":six", dict(bias=1)),
    (1, 0, 960, 4096, 512, "64/ns=1/xcd=0/fast", "", {}),                                        # 15 panels of 64 rows: no XCD map, f16 pieces
    (0, 1, 2048, 2048, 128, "64/ns=1/xcd=1/fast", ":six", {}),
    (0, 1, 2048, 2048, 256, "64/ns=1/xcd=1/fast", "", dict(pad=(4, 4, 4), bias=1)),              # 64-row tiles, each layout
    (0, 0, 2048, 2048, 256, "64/ns=1/xcd=1/fast", "", {}),
    (1, 0, 2048, 2048, 256, "64/ns=1/xcd=1/fast", "", dict(bias=2)),
    (1, 1, 2048, 2048, 256, "64/ns=1/xcd=1/fast", "", dict(pad=(4, 4, 0))),
]
NEW = (
    [R("fp32", ta, tb, M, N, K, "F32/" + l, **kw) for ta, tb, M, N, K, l, kw in _F32_LIKE]
    + [R("bf16", ta, tb, M, N, K, "BF16/" + l, **kw) for ta, tb, M, N, K, l, kw in _F32_LIKE]
    + [R("bf16x6", ta, tb, M, N, K, "SPLIT/" + l + "/thin?", **kw) for ta, tb, M, N, K, l, six, kw in _SPLIT]
    + [R("f16x3", ta, tb, M, N, K, "SPLIT/" + l + "/pieces" + six + "/thin?", **kw) for ta, tb, M, N, K, l, six, kw in _SPLIT]
    + [
        # the bounds-checked kernel: ragged edges, pitches dim + 1 and dim + 4, operands 4 bytes off a 16-byte boundary -- also on a shape whose
        # tiles are all interior -- every reducer it reaches, biases under split-K
        R("fp32", 1, 1, 129, 131, 33, "F32_EDGE/128/ns=1/xcd=0/thin?", pad=(1, 1, 1)),
        R("fp32", 0, 0, 130, 129, 50, "F32_EDGE/128/ns=1/xcd=0/thin?", pad=(4, 4, 4), off=(1, 0), bias=1),
        R("fp32", 0, 1, 128, 128, 64, "F32_EDGE/128/ns=1/xcd=0/thin?", off=(0, 1)),
        R("fp32", 1, 0, 128, 128, 64, "F32_EDGE/128/ns=1/xcd=0/thin?", pad=(1, 0, 0)),
        R("fp32", 0, 0, 30, 50, 40, "F32_EDGE/128/ns=1/xcd=0/thin?/skinny?", bias=1),
        R("fp32", 0, 1, 16384, 1536, 32, "F32_EDGE/128/ns=1/xcd=1/thin?", pad=(1, 1, 0)),
        R("fp32", 1, 0, 16390, 1530, 5, "F32_EDGE/128/ns=1/xcd=1/thin?/skinny?", bias=2),
        R("fp32", 1, 0, 70, 33, 300, "F32_EDGE/128/ns=5/xcd=0/thin?", reduce="SCALAR", pad=(1, 4, 1)),
        R("fp32", 1, 0, 70, 33, 3000, "F32_EDGE/128/ns=47/xcd=0/thin?", reduce="WAVE", bias=1),
        R("fp32", 1, 1, 200, 120, 1000, "F32_EDGE/128/ns=16/xcd=0/thin?", reduce="SCALAR", bias=2),
        R("f16x3", 0, 0, 20, 70, 300, "F32_EDGE/128/ns=5/xcd=0/thin?/skinny?", reduce="SCALAR", bias=1),
        R("f16x3", 0, 0, 2048, 192, 100, "F32_EDGE/128/ns=2/xcd=1/thin?", reduce="VEC1"),
        R("f16x3", 0, 0, 2048, 192, 100, "F32_EDGE/128/ns=2/xcd=1/thin?", reduce="SCALAR", bias=2),
        R("f16x3", 0, 1, 2050, 260, 260, "F32_EDGE/128/ns=3/xcd=1/thin?", reduce="SCALAR", pad=(1, 1, 3), bias=1),
        R("f16x3", 1, 1, 300, 100, 70, "F32_EDGE/64/ns=1/xcd=0/thin?", pad=(4, 1, 0)),
        R("f16x3", 1, 0, 300, 100, 20, "F32_EDGE/64/ns=1/xcd=0/thin?/skinny?", bias=1),
        R("f16x3", 0, 1, 1030, 200, 70, "F32_EDGE/64/ns=1/xcd=1/thin?", pad=(1, 1, 1), off=(1, 1), bias=2),
        R("f16x3", 0, 0, 1030, 200, 70, "F32_EDGE/64/ns=1/xcd=1/thin?"),
        R("f16x3", 1, 0, 1030, 200, 20, "F32_EDGE/64/ns=1/xcd=1/thin?/skinny?", pad=(4, 4, 4), bias=1),
        # thin.hip and skinny.hip behind pitched operands, operands 4 bytes off and a pitched C: their own guards decide (a pitched C or an
        # unaligned bias keeps the small-K kernel's 16-byte stores away: those fall through to the tile kernels, rows above)
        R("f16x3", 0, 0, 4096, 128, 3, "F32_EDGE/64/ns=1/xcd=0/thin?", via="thin", pad=(1, 1, 4), off=(1, 1), bias=1),
        R("f16x3", 0, 1, 4096, 3, 128, "F32_EDGE/128/ns=2/xcd=0/thin?", via="thin", pad=(4, 1, 1), off=(0, 1), bias=2),
        R("f16x3", 1, 0, 3, 128, 4096, "F32_EDGE/128/ns=64/xcd=0/thin?", via="thin", pad=(1, 4, 1), off=(1, 0)),
        R("f16x3", 0, 1, 17, 33, 100, "F32_EDGE/128/ns=2/xcd=0/thin?/skinny?", via="skinny", pad=(1, 1, 1), off=(1, 1), bias=2),
        R("fp32", 0, 0, 7, 50, 9, "F32_EDGE/128/ns=1/xcd=0/thin?/skinny?", via="skinny", pad=(4, 1, 4), off=(0, 1)),
        R("bf16x6", 1, 0, 70, 33, 3, "F32_EDGE/128/ns=1/xcd=0/thin?/skinny?", via="skinny", pad=(1, 4, 1), off=(1, 0)),
        # the 64-column kernel, in every mode and in its three layouts
        R("fp32", 0, 0, 128, 64, 32, "N64/128/ns=1/xcd=0/thin?"),
        R("bf16", 1, 0, 128, 64, 32, "N64/128/ns=1/xcd=0/thin?/skinny?", bias=1),
        R("bf16x6", 0, 1, 128, 64, 128, "N64/128/ns=2/xcd=0/thin?", reduce="VEC1"),
        R("f16x3", 1, 0, 256, 64, 4096, "N64/128/ns=64/xcd=0/thin?", reduce="VEC8", pad=(4, 4, 0)),
        R("fp32", 0, 0, 384, 64, 1024, "N64/128/ns=16/xcd=0/thin?", reduce="VEC4"),
        R("f16x3", 0, 1, 256, 64, 64, "N64/64/ns=1/xcd=0/thin?", pad=(4, 4, 4), bias=1),
        R("bf16x6", 1, 0, 256, 64, 32, "N64/64/ns=1/xcd=0/thin?/skinny?", bias=2),
        R("bf16", 0, 0, 512, 64, 96, "N64/64/ns=1/xcd=0/thin?"),
        # the folded weight gradient on the bf16 kernel, and in the default mode
        R("bf16", 1, 0, 64, 64, 8192, "FOLD64:BF16/128/ns=64/xcd=0/fast/thin?", via="fold", reduce="VEC8"),
        R("f16x3", 1, 0, 64, 64, 16384, "FOLD64:F32/128/ns=128/xcd=0/fast/thin?", via="fold", reduce="VEC8"),
        R("f16x3", 1, 0, 64, 64, 524288, "FOLD64:SPLIT/128/ns=256/xcd=0/fast/pieces:six/thin?", via="fold", reduce="VEC8"),
    ]
)

# the second integer tier of tests/test_gpu_gemm_variants.py (one operand up to 2^12: two pieces): rows of NEW on the split kernel whose K keeps
# every sum of |a b| below 2^24 -- both tile heights, each layout, one pass and split-K at xcd_map 0, 1 and 2, in both piece modes
PIECE_TIER = [r for r in NEW if r.label.startswith("SPLIT/") and r.K <= 1024 and r.M <= 4096]


def rows():
    """(test name, Row) of every launch"""
    return [(name, r) for name, rs in TESTS.items() for r in rs] + [("test_gpu_gemm_variants", r) for r in NEW]


def shapes(test, bias=False):
    """the distinct (ta, tb, M, N, K[, bias]) of a test's contiguous launches, in table order"""
    out = []
    for r in TESTS[test]:
        s = (r.ta, r.tb, r.M, r.N, r.K) + ((r.bias,) if bias else ())
        if r.pad == (0, 0, 0) and s not in out:
            out.append(s)
    return out


def pitches(r):
    return ((r.M if r.ta else r.K) + r.pad[0], (r.K if r.tb else r.N) + r.pad[1], r.N + r.pad[2])


def grid(r):
    """(grid_x, grid_y) of the tile launch of a row, from its label: gemm_plan_tiles' panel-major grid, the XCD-grouped ones, the N = 64 kernel's
    (test_gemm_plan_cpu.py holds it against the plan's)"""
    fam, bm, ns, xcd = parse(r.label)
    M, N = (128, 128) if r.via == "fold" else (r.M, r.N)
    ntm, ntn = -(-M // bm), -(-N // 128)
    if fam == "N64":
        return M // 128, ns
    if xcd == 1:
        return -(-ntm // 8) * 8 * ntn, ns
    if xcd in (2, 3):
        return ntm * ntn * ns, 1
    return ntm * ntn, ns


def parse(label):
    """-> (family, bm, ns, xcd_map) of a label (of the launch inside for FOLD64)"""
    f = label.split(":", 1)[1].split("/") if label.startswith("FOLD64:") else label.split("/")
    return f[0], int(f[1]), int(f[2][3:]), int(f[3][4:])
