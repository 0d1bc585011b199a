"""The shapes the kNN tests search, each with the kernel it reaches: (B, N, C, k, "family[/CT[/flags]]"), the label as
tools/knn_plan_host_check prints it for the plan (csrc/knn_plan.h) of that shape with contiguous 16-byte aligned rows and the planes
functional.knn_graph's workspace holds.  tests/test_knn_plan_cpu.py asserts every label against the plan and that the labels cover every
family / channel tile / v5 RES and KB the plan can return; tests/test_gpu_kernels.py searches the shapes on the GPU.

Families: VEX (knn6_kernel's vector-exact mode, C <= 3), V6/CT (knn6_kernel), V6W_V5/CT/v5=CT (knn6w_kernel with knn_mfma5_kernel behind it for
the clouds it flags), V5/CT (knn_mfma5_kernel; res: LDS-resident cloud, kb: the k > 24 variant), V4/CT (knn_mfma4_kernel: N >= 256, ragged),
V3/CT (knn_mfma3_kernel: small clouds, C > 128), VALU/KMAX (knn_kernel; c3: compile-time C = 3); vec: 16-byte row loads."""

# test_knn_bit_exact_vs_oracle
BIT_EXACT = [
    (2, 256, 3, 20, "VEX"), (2, 1024, 3, 20, "VEX"), (2, 256, 64, 20, "V6/64"), (1, 1024, 128, 20, "V6/128"),
    # small clouds (N < 128 or N < 256 at k <= 24) and C > 128 at k <= 32: lane-distributed lists
    (3, 20, 3, 20, "V3/4"), (2, 33, 64, 20, "V3/64/vec"), (2, 100, 5, 7, "V3/16"), (2, 70, 16, 1, "V3/16/vec"), (16, 128, 16, 20, "V3/16/vec"),
    (1, 100, 100, 20, "V3/128/vec"), (1, 100, 200, 20, "V3/256/vec"),
    # v4 (two-pass select, one wave per query group): N >= 256 that is no multiple of 128, k <= 32, C <= 128
    (1, 300, 3, 20, "V4/4"), (1, 300, 16, 20, "V4/16/vec"), (1, 300, 64, 20, "V4/64/vec"), (1, 300, 100, 20, "V4/128/vec"),
    # v5 (two waves per query group) at k <= 24: C <= 16 on whole chunks, LDS-resident / streamed, vector / scalar loads; wider clouds only
    # past v6's N <= 4096
    (2, 384, 16, 20, "V5/16/vec,res"), (3, 384, 5, 20, "V5/16/res"), (1, 4096, 16, 8, "V5/16/vec"), (1, 2048, 3, 20, "V5/4/res"),
    (1, 1152, 3, 20, "V5/4/res"), (1, 4736, 3, 20, "V5/4"), (1, 4224, 64, 20, "V5/64/vec"), (1, 4224, 128, 20, "V5/128/vec"),
    # v5 at k > 40 (128 chunk maxima per query), and at 24 < k <= 40 where the wide kernel does not stand in front
    (1, 256, 16, 48, "V5/16/vec,res,kb"), (1, 1152, 16, 48, "V5/16/vec,kb"), (1, 3584, 3, 48, "V5/4/kb"), (1, 128, 64, 64, "V5/64/vec,kb"),
    (2, 2048, 64, 64, "V5/64/vec,kb"), (1, 128, 128, 48, "V5/128/vec,kb"),
    # v6 (knn6.hip: k <= 24, N % 128 == 0, 16 < C <= 128, N <= 4096): the benchmarked shapes themselves (BASELINE.json configs[1]: B = 32,
    # N = 1024), fewest tiles, ragged tile-ring tails, k = 24, unaligned rows
    (32, 1024, 64, 20, "V6/64"), (32, 1024, 128, 20, "V6/128"), (32, 2048, 64, 20, "V6/64"), (1, 512, 100, 20, "V6/128"), (8, 128, 64, 20, "V6/64"),
    (9, 256, 128, 20, "V6/128"), (2, 128, 64, 24, "V6/64"), (2, 1152, 64, 20, "V6/64"), (2, 640, 33, 7, "V6/64"), (1, 2048, 128, 24, "V6/128"),
    # the vector-exact mode of v6: C <= 3, N <= 1024, k = 1 / 24
    (32, 1024, 3, 20, "VEX"), (1, 128, 3, 1, "VEX"), (2, 256, 3, 24, "VEX"),
    # v6 wide (knn6w_kernel: 24 < k <= 40, N % 128 == 0, every C <= 128 that v5 takes) with v5 behind it: one tile per quarter, ragged
    # rings, the configs[4] shape (k = 40)
    (2, 256, 5, 32, "V6W_V5/16/v5=16,res"), (1, 1152, 16, 40, "V6W_V5/16/v5=16,vec"), (2, 2048, 3, 40, "V6W_V5/16/v5=4,res"), (1, 3584, 3, 40, "V6W_V5/16/v5=4"),
    (2, 640, 64, 32, "V6W_V5/64/v5=64,vec"), (8, 2048, 64, 40, "V6W_V5/64/v5=64,vec"), (2, 512, 64, 33, "V6W_V5/64/v5=64,vec"), (2, 1024, 64, 25, "V6W_V5/64/v5=64,vec"),
    (2, 128, 64, 40, "V6W_V5/64/v5=64,vec"), (3, 256, 64, 25, "V6W_V5/64/v5=64,vec"), (1, 1152, 33, 37, "V6W_V5/64/v5=64"), (16, 2048, 64, 40, "V6W_V5/64/v5=64,vec"),
    (1, 4096, 64, 40, "V6W_V5/64/v5=64,vec"), (3, 1024, 128, 40, "V6W_V5/128/v5=128,vec"), (2, 640, 128, 40, "V6W_V5/128/v5=128,vec"),
    # the VALU kernel: 32 < k <= 40 on shapes outside the two-pass kernels (ragged N, N < 128, 64 < C < 128 with k > 24, C > 128)
    (1, 300, 3, 40, "VALU/40/c3"), (1, 384, 100, 40, "VALU/40"), (2, 150, 200, 40, "VALU/40"), (1, 96, 200, 36, "VALU/40"), (2, 100, 24, 33, "VALU/40"),
]

# the other kNN tests of tests/test_gpu_kernels.py and smoke(): test -> (B, N, C, k, ld, label) of every search it makes
OTHER = {
    "test_knn_duplicates_and_strided_input": [(1, 64, 3, 20, 3, "V3/4"), (2, 128, 64, 20, 96, "V6/64")],
    "test_knn_near_duplicates_need_exact_distances": [
        (3, 512, 3, 20, 3, "VEX"), (3, 512, 64, 20, 64, "V6/64"), (3, 512, 128, 20, 128, "V6/128"), (3, 512, 3, 40, 3, "V6W_V5/16/v5=4,res"),
        (3, 512, 64, 40, 64, "V6W_V5/64/v5=64,vec"), (3, 512, 128, 40, 128, "V6W_V5/128/v5=128,vec")],
    "test_knn_clouds_far_from_the_origin": [
        (4, 1024, 64, 20, 64, "V6/64"), (2, 1024, 128, 20, 128, "V6/128"), (2, 512, 64, 20, 64, "V6/64"), (2, 1024, 3, 20, 3, "VEX"),
        (4, 1024, 64, 40, 64, "V6W_V5/64/v5=64,vec"), (2, 1024, 128, 40, 128, "V6W_V5/128/v5=128,vec"), (2, 512, 64, 40, 64, "V6W_V5/64/v5=64,vec"),
        (2, 1024, 3, 40, 3, "V6W_V5/16/v5=4,res")],
    "test_knn_nonfinite_rows_do_not_poison_the_others": [(2, 256, 3, 20, 3, "VEX")],
    "test_knn_nan_rows_are_defined_and_in_range": [
        (3, 256, 3, 20, 3, "VEX"), (3, 256, 64, 20, 64, "V6/64"), (3, 256, 128, 20, 128, "V6/128"), (3, 256, 64, 40, 64, "V6W_V5/64/v5=64,vec"),
        (3, 256, 3, 40, 3, "V6W_V5/16/v5=4,res")],
    "test_knn_massive_ties_overflow_path": [
        (2, 256, 16, 20, 16, "V5/16/vec,res"), (2, 256, 16, 28, 16, "V6W_V5/16/v5=16,vec,res"), (2, 256, 16, 40, 16, "V6W_V5/16/v5=16,vec,res"),
        (2, 256, 16, 64, 16, "V5/16/vec,res,kb"), (1, 256, 3, 20, 3, "VEX"), (1, 256, 3, 28, 3, "V6W_V5/16/v5=4,res"), (1, 256, 3, 40, 3, "V6W_V5/16/v5=4,res"),
        (1, 256, 3, 64, 3, "V5/4/res,kb")],
    "test_knn_public_api_and_errors": [(2, 128, 3, 20, 3, "VEX")],
    "test_knn_two_pass_overflow_fallback": [(3, 512, 3, 20, 3, "VEX"), (2, 1024, 64, 20, 64, "V6/64"), (2, 300, 3, 20, 3, "V4/4"), (1, 300, 64, 20, 64, "V4/64/vec")],
    "test_knn_wide_mixed_clouds_flag_handover": [(4, 256, 64, 40, 64, "V6W_V5/64/v5=64,vec")],
    "test_knn_counting_final_without_list_overflow": [(1, 384, 64, 20, 64, "V6/64"), (1, 384, 64, 40, 64, "V6W_V5/64/v5=64,vec")],
    "smoke": [(4, 128, 3, 20, 3, "VEX")],
}

# test_knn_golden_reference_rows: fixture -> label (B and k are the fixture's own)
GOLDEN = {"knn_s0_C3_N256.npz": "VEX", "knn_s1_C3_N1024.npz": "VEX", "knn_s2_C64_N256.npz": "V6/64", "knn_s3_C128_N1024.npz": "V6/128",
          "knn_s4_C3_N20.npz": "V3/4", "knn_s5_C64_N33.npz": "V3/64/vec"}
