/* libmlsp_hip.so -- C ABI of the MI355X (gfx950) hot path of MLSP.
 *
 * The reference (VITA-Group/MLSP) has no FFI/operator interface of its own: its boundary is the
 * Python nn.Module / free-function surface of PointDA/Models.py, PointDA/model_utils.py and
 * MLSP/mlsp.py.  This header is the native boundary underneath the Python
 * mirror of that surface (mlsp_amd/Models.py, model_utils.py, mlsp.py): each entry point names
 * the reference code it replaces.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch tensors); the library never
 *     allocates or frees caller-visible memory.  Scratch is passed in (`ws`, `ws_bytes`; size it
 *     with mlsp_workspace_bytes).
 *   - every compute call is asynchronous on `stream`, re-entrant, never throws, and returns 0 on
 *     success, a negative MLSP_ERR_* code for bad arguments, or a positive hipError_t.  The compute
 *     entry points keep no mutable state: what a call does is a function of its arguments alone, from any thread, on any stream
 *     (ABI v8: the products of the GEMM family are the per-call `precision` argument below, not a library switch; ABI v13:
 *     mlsp_operand_bounds_next hands ONE following call an optional table through a thread-local slot -- the library's only one -- that
 *     the next entry point with a `precision` empties as its first act, a shape query or a call it rejects included: an out-of-band
 *     argument of that call, not state.  Inside, the call's mode, operand bounds and table travel as one explicit context object).  The only process-wide object is the measurement hook mlsp_profile_begin/_end (HIP events around launches while armed; bench.py only,
 *     never armed in a production step).  The library reads one environment variable, MLSP_PROF_DUMP (a listing of
 *     the profiled launches while the hook is armed); it changes no kernel choice.
 *   - `precision` (every entry point that reaches a matrix-core contraction takes it, just before its workspace):
 *       MLSP_PREC_F32    0  f32 MFMA, exact fp32 products (v_mfma_f32_32x32x2_f32);
 *       MLSP_PREC_BF16   1  operands ROUNDED to bf16, fp32 accumulation (BASELINE.json configs[4]; reduced precision);
 *       MLSP_PREC_BF16X6 2  fp32-ACCURATE products on the bf16 matrix cores: every operand value split exactly into three bf16 pieces
 *                           (8 + 8 + 8 significand bits), six piece products per multiply, fp32 accumulation.  Against float64 its error
 *                           is below the f32-MFMA chain's (tests/test_gpu_kernels.py::test_gemm_split_bf16_accuracy), 1.55-1.65x faster
 *                           on the 32768-row layers.  The mode of every number bench.py reported in rounds 3-5 (its `bf16x6_split`
 *                           leg since).  An infinite operand becomes NaN (the f32 MFMA would give +-inf).
 *       MLSP_PREC_F16X3  3  (ABI v13) the same accuracy class with HALF the matrix work: two f16 pieces per operand value under a
 *                           per-workgroup power-of-two scale, three piece products (see the definition below).  THE MODE OF EVERY NUMBER
 *                           bench.py REPORTS since round 6 and the default of the Python mirror (MLSP_GEMM_PRECISION overrides it there).
 *     Launches off the interior-tile path, short K loops, operand-transform and N = 64 launches run on the f32 kernels in every mode
 *     (exact fp32 either way); kNN distances, BatchNorm statistics, reductions and losses are fp32 in every mode.  A backward call
 *     normally passes the precision of its forward (the Python mirror keeps it in the autograd context); nothing breaks if it differs.
 *   - activations are POINT-major fp32 row matrices: [rows][C] with rows = B*N points (or
 *     B*N*k edges), channels contiguous.  The reference itself moves to this layout before its
 *     gather (model_utils.py:35).  Indices are int32, local to their cloud (0..N-1).
 *   - act: 0 none, 1 ReLU, 2 LeakyReLU(slope).
 *   - bn_save is [4][C] floats: scale (= gamma*invstd), shift (= beta - mean*scale), mean, invstd.
 */
#ifndef MLSP_HIP_H
#define MLSP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* mlsp_stream_t; /* == hipStream_t */

#define MLSP_ABI_VERSION 14
#define MLSP_OK 0
#define MLSP_ERR_ARG (-1)
#define MLSP_ERR_WORKSPACE (-2)
#define MLSP_ERR_UNSUPPORTED (-3)
#define MLSP_PREC_F32 0
#define MLSP_PREC_BF16 1
#define MLSP_PREC_BF16X6 2
/* ABI v13.  fp32-accurate products on the f16 matrix cores with HALF the matrix work of MLSP_PREC_BF16X6: every fp32 operand value, times a
 * per-workgroup power of two, is split into two f16 pieces (11 + 11 significand bits) and a product is three piece products with fp32
 * accumulation.  The scale comes from a bound of the operand's magnitude: measured (one streaming launch per operand and call, partial
 * maxima in the last 64 KiB of the call's workspace) or analytic (an operand that is transformed by batch-statistics BatchNorm on the fly);
 * a launch without a bound (no workspace tail, eval-mode transform) runs the six-product bf16 split instead.  Same accuracy class as
 * MLSP_PREC_BF16X6 (tests/test_gpu_kernels.py::test_gemm_split_bf16_accuracy holds both to the same bar against float64). */
#define MLSP_PREC_F16X3 3
/* Caller-owned operand bounds for MLSP_PREC_F16X3 (optional; ABI v13).  partials: 256 floats on the device -- partial maxima of |X| over X
 * [rows][cols] (row pitch ld, fp32, 16-byte aligned, cols % 4 == 0).  mlsp_operand_bounds_next(tab, n) hands `n` entries to the NEXT entry
 * point this thread calls that takes a `precision` (and to that call only; the table must stay alive until it returns): a GEMM operand of
 * that call with the same pointer and shape uses the entry's partials instead of measuring into the workspace -- as they are when
 * valid != 0; when valid == 0 the call measures INTO them (its one measuring launch) and sets valid = 1 in the caller's table.  The caller
 * keeps such a buffer for as long as the tensor's contents do not change: an activation that several layers read, a weight that its
 * layer's backward reads again.  A VALID entry may hold any number n <= 4096 of partials from any source whose maximum bounds |X| -- e.g. the
 * per-tile maxima mlsp_adam_flat_f32 leaves of the parameters it just updated.  Purely an optimisation: without it every call measures
 * what it needs. */
typedef struct { const float* ptr; long rows; int cols, ld; float* partials; int valid; int n; } mlsp_bound_t;   /* n: partials held (0 = 256); an entry to be measured (valid == 0) holds 256 */
int mlsp_operand_bounds_next(mlsp_bound_t* tab, int n);

int mlsp_abi_version(void);
const char* mlsp_strerror(int code);

/* Upper bound of the scratch bytes any entry point needs for a problem with `rows` activation
 * rows, `cin`/`cout` channels (pass the largest of each used with one workspace). */
size_t mlsp_workspace_bytes(int rows, int cin, int cout);

/* knn(x,k): PointDA/model_utils.py:9-16 (twin PointSegDA/Models.py:8-15).
 * x [B][N] rows of C floats with row pitch ldx; idx [B][N][k], nearest first (canonical arithmetic,
 * see oracle/knn_canon.c).  If rev_off != NULL also builds the reverse neighbour index used by the
 * backward passes: rev_off [B*N+1], rev_ent [B*N*k] packed (i_local << 8 | slot), sorted. */
int mlsp_knn_f32(const float* x, int ldx, int B, int N, int C, int k, int32_t* idx, int32_t* rev_off, int32_t* rev_ent,
                 void* ws, size_t ws_bytes, mlsp_stream_t stream);

/* reverse neighbour index alone, for caller-provided indices (get_graph_feature(..., idx=...)) */
int mlsp_knn_reverse(const int32_t* idx, int B, int N, int k, int32_t* rev_off, int32_t* rev_ent, mlsp_stream_t stream);

/* get_graph_feature(x,args,k,idx): PointDA/model_utils.py:18-42, materialised edge-major:
 * F [B*N*k][2C] = [x_j - x_i ; x_i].  (The reference's [B,2C,N,k] result is a permuted view of this.) */
int mlsp_graph_feature_fwd_f32(const float* x, const int32_t* idx, int B, int N, int C, int k, float* F, mlsp_stream_t stream);
int mlsp_graph_feature_bwd_f32(const float* dF, const int32_t* rev_off, const int32_t* rev_ent, int B, int N, int C, int k,
                               float* dx, mlsp_stream_t stream);

/* Fused EdgeConv block = get_graph_feature + conv_2d (1x1 Conv2d bias=False + BatchNorm2d + act) + max over k:
 * PointDA/model_utils.py:18-63 with PointDA/Models.py:115-129.  Algebraically folded (edge.hip).
 * W [Cout][2C] in the reference's Conv2d layout.  Saved for backward: uv [P][2Cout], msel [P][Cout] (the selected edge's
 * pre-BatchNorm value y = v_i + the extreme of u_j over the neighbours: the sum, not the extreme alone),
 * argsel [P][Cout] u8, s1 [P][Cout], bn_save [4][Cout].  out (row pitch ldo >= Cout) and dOut (row pitch lddo) may be column
 * slices of a wider matrix: the four EdgeConv outputs are written straight into the [P][512] concatenation of
 * PointDA/Models.py:131 (no torch.cat pass) and its gradient is read in place.
 * Wd [2Cout][C] (nullable): the folded weight [Wa ; Wb - Wa] the forward builds anyway; a caller that keeps it and hands it to the
 * backward saves the rebuild.  dx (row pitch lddx >= C) may be a column slice as well, and with dx_accumulate != 0 the input
 * gradient is ADDED to it: layer l+1 adds its input gradient into layer l's slice of the concatenation's gradient, which is the
 * sum autograd would otherwise form with a separate pass. */
int mlsp_edgeconv_fwd_f32(const float* x, int ldx, const int32_t* idx, const float* W, const float* gamma, const float* beta,
                          float* run_mean, float* run_var, float momentum, float eps, int act, float slope, int training,
                          int B, int N, int C, int Cout, int k, float* out, int ldo, float* uv, float* msel, uint8_t* argsel,
                          float* s1, float* bn_save, float* Wd, int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_edgeconv_bwd_f32(const float* dOut, int lddo, const float* x, int ldx, const int32_t* rev_off, const int32_t* rev_ent,
                          const float* W, const float* out, int ldo, const float* uv, const float* msel, const uint8_t* argsel,
                          const float* s1, const float* bn_save, const float* Wd, int act, float slope, int training, int B, int N,
                          int C, int Cout, int k, float* dx, int lddx, int dx_accumulate, float* dW, float* dgamma, float* dbeta,
                          int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);

/* Fused per-edge stage of the T-Net (PointDA/model_utils.py:111-115: conv2d1 6->64, conv2d2 64->128 per EDGE, max over k),
 * dgcnn branch (bias-free convs, LeakyReLU).  x [P][C] point-major (C = 3), W1 [C1][2C], W2 [C2][C1]; requires C1 = 64, C2 = 128
 * (returns MLSP_ERR_UNSUPPORTED otherwise: use graph_feature + pointmlp + segmax).  out [P][C2].
 * Saved for backward: uv [P][2*C1], s1 [P][C1], bn1_save [4][C1], zsel [P][C2], argsel [P][C2] u8, bn2_save [4][C2]. */
int mlsp_tnet_edge_fwd_f32(const float* x, int ldx, const int32_t* idx, const float* W1, const float* gamma1, const float* beta1,
                           float* run_mean1, float* run_var1, const float* W2, const float* gamma2, const float* beta2,
                           float* run_mean2, float* run_var2, float momentum, float eps, float slope, int training, int B, int N,
                           int C, int C1, int C2, int k, float* out, float* uv, float* s1, float* bn1_save, float* zsel,
                           uint8_t* argsel, float* bn2_save, int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_tnet_edge_bwd_f32(const float* dOut, const float* x, int ldx, const int32_t* idx, const int32_t* rev_off,
                           const int32_t* rev_ent, const float* W1, const float* W2, const float* out, const float* uv,
                           const float* s1, const float* bn1_save, const float* zsel, const uint8_t* argsel, const float* bn2_save,
                           float slope, int training, int B, int N, int C, int C1, int C2, int k, float* dx, float* dW1,
                           float* dgamma1, float* dbeta1, float* dW2, float* dgamma2, float* dbeta2, int precision, void* ws, size_t ws_bytes,
                           mlsp_stream_t stream);

/* Per-row MLP layer = Linear/1x1 conv (+bias) + BatchNorm + act + dropout:
 * conv_2d / fc_layer (model_utils.py:45-87), conv5+bn5 (Models.py:132), head layers (Models.py:192-196,
 * 226-230, 272-279).  W [Cout][Cin] with row pitch ldw (a column slice of a wider weight is legal).  gbias [G][Cout] (nullable) is a per-row-group bias (row r uses group r / rows_per_group):
 * the x5-repeat half of the heads' 1536-channel input enters as a per-cloud bias (Models.py:156-160).
 * Y = pre-BN (saved), Z = output.  gamma == NULL: no BN (Y is not written, Z = act(linear)).
 * Backward: dx_accumulate != 0 adds the input gradient to what dX already holds (beta = 1 in the dgrad epilogue): the four consumers
 * of the concatenated encoder features (conv5 and the three heads, Models.py:132,156-160) sum their gradients in one buffer instead of
 * three 67 MB element-wise adds.
 * Chained layers (the output of a Linear+BN+act layer feeds only other such layers: conv1 -> conv2 -> conv3 -> conv4 of the heads,
 * Models.py:192-197): the producer is called with Z == NULL (only Y, the pre-BN output, and bn_save are written: the streaming
 * BN+act pass is skipped), the consumer through mlsp_pointmlp_fwd_chain_f32 / mlsp_pointmlp_bwd_chain_f32 with Xpre pointing at its
 * input columns inside the producer's Y and an mlsp_defer_t that describes the producer: act(Xpre * scale + shift) and the dropout mask
 * are applied while the GEMM stages the operand (forward: A rows; wgrad: the k-major B operand) -- on the split-product kernel, the f32
 * MFMA kernel and the streaming kernels of the 3 / 16-channel output layers alike, bit-identical to the product over the materialised
 * tensor -- or by one streaming pass into the workspace for shapes outside those kernels.  The gradients the consumer returns in dX are
 * with respect to the ACTIVATED input, i.e. exactly the dZ the producer's backward expects. */
typedef struct mlsp_defer {
    const float* bn_save;  /* the producer's [4][ld]: scale | shift | mean | invstd (device) */
    int ld;                /* the producer's width: row pitch of its Y and of bn_save; its dropout stream is indexed row * ld + column */
    int col;               /* first column of THIS consumer's input inside the producer's Y (Xpre == Y + col) */
    int act;               /* the producer's activation on these columns: 0 none, 1 ReLU, 2 LeakyReLU(slope) */
    float slope;
    float p_drop;          /* its dropout rate on these columns (0: none / eval mode) */
    uint64_t seed;         /* ... and the seed of that dropout stream */
} mlsp_defer_t;
int mlsp_pointmlp_fwd_f32(const float* X, int ldx, int M, int Cin, const float* W, int ldw, int Cout, const float* bias,
                          const float* gbias, int rows_per_group, const float* gamma, const float* beta, float* run_mean,
                          float* run_var, float momentum, float eps, int training, int act, float slope, float p_drop,
                          uint64_t seed, float* Y, float* Z, float* bn_save, float* group_ysum, int precision, void* ws, size_t ws_bytes,
                          mlsp_stream_t stream);
int mlsp_pointmlp_fwd_chain_f32(const float* Xpre, int ldx, const mlsp_defer_t* in, int M, int Cin, const float* W, int ldw, int Cout, const float* bias,
                                const float* gbias, int rows_per_group, const float* gamma, const float* beta, float* run_mean,
                                float* run_var, float momentum, float eps, int training, int act, float slope, float p_drop,
                                uint64_t seed, float* Y, float* Z, float* bn_save, float* group_ysum, int precision, void* ws, size_t ws_bytes,
                                mlsp_stream_t stream);
/* BatchNorm-backward reduction fused into the consumer's dgrad (round 5).  The gradient w.r.t. a chained layer's activated output is
 * produced by its CONSUMER's dgrad; that launch (gemm_split_kernel's output pass, the small-K streaming kernel) can multiply it by the
 * producer's activation derivative and dropout mask right there, store the masked gradient d' and leave the producer's column sums of
 * d' and d' * yhat per 128-row panel: the producer's streaming reduction pass (a full read of dZ and Y) disappears.
 *   consumer: in_stats != NULL ([M / 128][2][in->ld] doubles, indexed by the producer's column, FOLLOWED (ABI v13) by [M / 128][in->ld]
 *             floats: the panels' column maxima of |d'|, a bound the producer's two-piece f16 products need) -- legal when
 *             mlsp_*_bwd_stats_parts() > 0 for the layer; dX then holds d', not dZ;
 *   producer: pre_stats != NULL ([pre_parts][2][Cout] doubles + [pre_parts][Cout] floats, as the consumers left them) -- dZ is d', its sums
 *             are given: finalisation + the BatchNorm part only;
 *             pre_stats == NULL with pre_parts < 0 (ABI v13) -- dZ is d' but its sums are INCOMPLETE: only some consumers took part in this
 *             backward pass (a loss on a subset of the heads, PointDA/trainer.py:551-565), the columns of the others are zero.  The
 *             call reduces the sums itself and does not apply the activation derivative / dropout mask a second time.
 * All consumers of a producer must be ABLE to do it or none does (they write columns of the same dX and of the same partial rows); the
 * ones that run in a given backward pass then all do it.
 * A producer in that role (training mode) does not form its output gradient dY either when its dgrad and weight-gradient launches run on
 * gemm_split_kernel: they read d' and Y and apply dY = (d' + y * nk2[c] + c0[c]) * sc[c] in their operand loads (coefficients from the
 * finalised sums), so the streaming "apply" pass and the dY tensor are gone; the per-cloud bias gradient (gbias) then comes from the panel
 * sums of d' and the clouds' column sums of Y -- group_ysum [n_groups][Cout], which the forward leaves when asked (nullable on both
 * sides: without it the backward takes one pass over Y).  Other shapes keep the apply pass (same results to rounding). */
int mlsp_pointmlp_bwd_stats_parts(int M, int Cin, int Cout, int ldw, int lddx, int precision);
int mlsp_pointmlp_bwd_chain_f32(const float* dZ, const float* Xpre, int ldx, const mlsp_defer_t* in, int M, int Cin, const float* W, int ldw, int Cout, const float* Y,
                                const float* bn_save, int has_bn, int training, int act, float slope, float p_drop, uint64_t seed,
                                int n_groups, int rows_per_group, float* dX, int lddx, int dx_accumulate, float* dW, float* dbias,
                                float* dgbias, float* dgamma, float* dbeta, double* in_stats, const double* pre_stats, int pre_parts,
                                const float* group_ysum, int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_pointmlp_bwd_f32(const float* dZ, const float* X, int ldx, int M, int Cin, const float* W, int ldw, int Cout, const float* Y,
                          const float* bn_save, int has_bn, int training, int act, float slope, float p_drop, uint64_t seed,
                          int n_groups, int rows_per_group, float* dX, int lddx, int dx_accumulate, float* dW, float* dbias, float* dgbias,
                          float* dgamma, float* dbeta, const double* pre_stats, int pre_parts, const float* group_ysum, int precision, void* ws,
                          size_t ws_bytes, mlsp_stream_t stream);

/* The same layer with its ACTIVATIONS stored as bf16 in HBM (BASELINE.json configs[4]: PointSegDA N=2048 k=40 "bf16 with MFMA edge-MLP";
 * PointSegDA/Models.py:245-385 head stacks).  x_bf16: X and dX are bf16 (else fp32); out_bf16: Y, Z, dZ and the internal dY are bf16.
 * W, bias, gbias, BatchNorm parameters / statistics, dW and every reduction stay fp32; products are bf16 x bf16 with fp32 accumulation.
 * BN layers on interior GEMM tiles only: mlsp_pointmlp_mx_supported() != 0, otherwise both entry points return MLSP_ERR_UNSUPPORTED and
 * the caller runs that layer through mlsp_pointmlp_*_f32. */
int mlsp_pointmlp_mx_supported(int M, int Cin, int Cout, int ldx, int x_bf16, int training, int precision);
int mlsp_pointmlp_fwd_mx(const void* X, int x_bf16, int ldx, int M, int Cin, const float* W, int ldw, int Cout, const float* bias,
                         const float* gbias, int rows_per_group, const float* gamma, const float* beta, float* run_mean,
                         float* run_var, float momentum, float eps, int training, int act, float slope, float p_drop, uint64_t seed,
                         void* Y, void* Z, int out_bf16, float* bn_save, int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_pointmlp_bwd_mx(const void* dZ, const void* X, int x_bf16, int ldx, int M, int Cin, const float* W, int ldw, int Cout,
                         const void* Y, int out_bf16, const float* bn_save, int training, int act, float slope, float p_drop,
                         uint64_t seed, int n_groups, int rows_per_group, void* dX, int lddx, int dx_accumulate, float* dW, float* dbias,
                         float* dgbias, float* dgamma, float* dbeta, int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);

/* Fused per-point conv (bias-free) + BatchNorm + act + max over the N points of each cloud:
 * conv5/bn5/LeakyReLU/adaptive_max_pool1d (PointDA/Models.py:132-136) and the T-Net's conv2d3 + torch.max(dim=2)
 * (PointDA/model_utils.py:116-117).  out [B][Cout].  Backward is closed-form through the Gram matrix X^T X (colmax.hip):
 * the dense [P][Cout] gradient is never formed.  Saved: ysel [B][Cout], arg [B][Cout], bn_save [4][Cout].  X must be
 * contiguous (ldx == Cin) for the backward.  arg is always in [0, N): a column of a cloud whose Y is all NaN names row 0.
 * mlsp_pointmlp_colmax_panel_rows (ABI v14; a shape query like mlsp_pointmlp_bwd_stats_parts, launches nothing): the height (64 or 128) of
 * the row panels whose column extremes the forward takes in its GEMM epilogue for this shape and product mode -- Y is then never written,
 * N / rows panels per cloud are merged --, or 0 when the forward writes Y and selects in a pass of its own. */
int mlsp_pointmlp_colmax_panel_rows(int B, int N, int Cin, int Cout, int precision);
int mlsp_pointmlp_colmax_fwd_f32(const float* X, int ldx, int B, int N, int Cin, const float* W, int ldw, int Cout,
                                 const float* gamma, const float* beta, float* run_mean, float* run_var, float momentum, float eps,
                                 int training, int act, float slope, float* out, float* ysel, int32_t* arg, float* bn_save, int precision, void* ws,
                                 size_t ws_bytes, mlsp_stream_t stream);
int mlsp_pointmlp_colmax_bwd_f32(const float* dOut, const float* X, int ldx, int B, int N, int Cin, const float* W, int ldw,
                                 int Cout, const float* out, const float* ysel, const int32_t* arg, const float* bn_save,
                                 int training, int act, float slope, float* dX, int dx_accumulate, float* dW, float* dgamma, float* dbeta,
                                 int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);

/* Several Linear (+bias) layers side by side under ONE BatchNorm + activation (+dropout) pass: layer d of the three MLSP heads
 * (PointDA/Models.py:193-196 position, :227-230 normal, :274-279 cardinality) in one [M][sum Cout] matrix.  Segment s:
 *   Y[:, y_s : y_s + Cout_s] = X[:, x_col_s : x_col_s + Cin_s] W_s^T (+ bias_s),   y_s = Cout_0 + ... + Cout_{s-1}
 * gamma / beta / running statistics / dgamma / dbeta / dbias are [C] vectors over all the channels (C = sum Cout <= 1024), bn_save
 * [4][C].  chan [2][C]: per channel the negative-side factor of the activation max(a, f a) (0 ReLU, 0.2 LeakyReLU, 1 none) and the
 * dropout switch (0 / 1; rate p_drop, counter hash of element row * C + channel).  `segs` and `dW` (one [Cout_s][Cin_s] gradient per
 * segment) are HOST arrays.  Backward: dX [M][..] (row pitch lddx; nullable) gets segment s's input gradient in columns x_col_s..;
 * segments reading the same columns add up.  MLSP_ERR_UNSUPPORTED (mlsp_multimlp_supported() == 0) when a column slice is not
 * 16-byte aligned or C > 1024: run one mlsp_pointmlp_* per segment instead.
 * Chaining (ABI v9): `in` (HOST array of nseg descriptors, or NULL) says that X is the PRE-BatchNorm output of the previous merged layer
 * (in[s].col == segs[s].x_col): every segment's GEMM -- single or block-diagonal -- transforms its operand while staging it (forward:
 * A; backward: the X side of the weight gradient), see mlsp_defer_t above.  Z == NULL in the forward: this layer's own BatchNorm +
 * activation + dropout pass is left to ITS consumers (Y and bn_save are written). */
typedef struct mlsp_seg {
    const float* W;        /* [Cout][Cin], row pitch ldw */
    const float* bias;     /* [Cout] or NULL */
    int ldw, x_col, Cin, Cout;
} mlsp_seg_t;
int mlsp_multimlp_supported(int M, const mlsp_seg_t* segs, int nseg, int precision);
int mlsp_multimlp_fwd_f32(const float* X, int ldx, int M, const mlsp_seg_t* segs, int nseg, const mlsp_defer_t* in, const float* gamma, const float* beta,
                          float* run_mean, float* run_var, float momentum, float eps, int training, const float* chan, float p_drop,
                          uint64_t seed, float* Y, float* Z, float* bn_save, int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_multimlp_bwd_stats_parts(int M, const mlsp_seg_t* segs, int nseg, int ldx, int lddx, int precision);
int mlsp_multimlp_bwd_f32(const float* dZ, const float* X, int ldx, int M, const mlsp_seg_t* segs, int nseg, const mlsp_defer_t* in, const float* Y,
                          const float* bn_save, int training, const float* chan, float p_drop, uint64_t seed, float* dX, int lddx,
                          float* const* dW, float* dbias, float* dgamma, float* dbeta, double* in_stats, const double* pre_stats, int pre_parts,
                          int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);

/* max over the k edges of every point (`.max(dim=-1)`, model_utils.py:114) on an edge-major matrix */
int mlsp_segmax_fwd_f32(const float* Z, int P, int k, int C, float* out, uint8_t* argk, mlsp_stream_t stream);
int mlsp_segmax_bwd_f32(const float* dOut, const uint8_t* argk, int P, int k, int C, float* dZ, mlsp_stream_t stream);

/* max over the N points of every cloud (model_utils.py:117 torch.max(dim=2); Models.py:136 adaptive_max_pool1d) */
int mlsp_colmax_fwd_f32(const float* Z, int B, int N, int C, float* out, int32_t* arg, mlsp_stream_t stream);
int mlsp_colmax_bwd_f32(const float* dOut, const int32_t* arg, int B, int N, int C, float* dZ, mlsp_stream_t stream);

/* masked symmetric Chamfer (MLSP/mlsp.py:115-182, scaled as calc_loss :222-229):
 * loss = scale * sum_b (A_b + B_b)/cnt_b,  scale = DefRec_weight * DefRec_SCALER / B.
 * pred [B][N][3], gold [B][3][N], mask [B][3][N]; per_cloud [B][3], argA/argB [B][N] saved.
 * Contract of both Chamfer forwards (this one and mlsp_chamfer_dir_fwd_f32):
 *  - the mask holds 0 or 1 (row 0 of [B][3][N] is read here); any non-zero entry counts as a masked row with no penalty.
 *  - on every masked row the stored arg-min column is in [0, N), whatever the inputs hold, so the backward never indexes outside
 *    the cloud.  The lowest column wins ties.
 *  - a masked point that is NaN or infinite, or coordinates so large that every squared distance of a masked row overflows, leave
 *    that row with no column below the start value: its minimum is stored as +inf, its arg as column 0, and the loss is non-finite.
 *  - a non-finite value in an UNMASKED point is not reported: such a column is never the nearest and such a row is never scanned,
 *    where the reference's 0 * NaN would make the loss NaN.  A known, accepted difference. */
int mlsp_chamfer_masked_fwd_f32(const float* pred, const float* gold, const float* mask, int B, int N, float scale,
                                float* per_cloud, int32_t* argA, int32_t* argB, float* loss, mlsp_stream_t stream);
int mlsp_chamfer_masked_bwd_f32(const float* pred, const float* gold, const float* mask, int B, int N, float scale,
                                const float* per_cloud, const int32_t* argA, const int32_t* argB, const float* grad_loss,
                                float* dpred, mlsp_stream_t stream);

/* ONE direction of the masked Chamfer distance = the reference's chamfer_distance(p1, p2, mask) (MLSP/mlsp.py:115-153):
 * loss = sum_b (sum over the masked rows i of p1 of min_j (|p1_i - p2_j|^2 + 100 [mask_j == 0])) / cnt_b.
 * p1, p2 [B][N][3]; mask_cord [B][N] = mask[:, :, 0]; per_cloud [B][2] = {sum, cnt} and arg [B][N] (arg-min column of every
 * masked row) are saved for the backward, which writes dp1 and / or dp2 [B][N][3] (either may be NULL).  The mask is 0/1 and arg
 * is in [0, N) on every masked row; non-finite points as stated for mlsp_chamfer_masked_fwd_f32 above. */
int mlsp_chamfer_dir_fwd_f32(const float* p1, const float* p2, const float* mask_cord, int B, int N, float* per_cloud, int32_t* arg,
                             float* loss, mlsp_stream_t stream);
int mlsp_chamfer_dir_bwd_f32(const float* p1, const float* p2, const float* mask_cord, int B, int N, const float* per_cloud,
                             const int32_t* arg, const float* grad_loss, float* dp1, float* dp2, mlsp_stream_t stream);

/* normal loss (MLSP/mlsp.py:275-287; weighted form PointDA/trainer.py:551-556):
 * out[0] = -weight * sum_i w_i |cos(pred_i, gt_i)| / sum_i w_i ; out[1] = sum w.  w nullable (=1). */
int mlsp_normal_loss_fwd_f32(const float* pred, const float* gt, const float* w, int P, float weight, float* out, void* ws,
                             size_t ws_bytes, mlsp_stream_t stream);
int mlsp_normal_loss_bwd_f32(const float* pred, const float* gt, const float* w, int P, float weight, const float* fwd_out,
                             const float* grad_loss, float* dpred, mlsp_stream_t stream);

/* cardinality-head tail (PointDA/Models.py:281-285): p = softmax(logits), density = p . fc2w */
int mlsp_density_tail_fwd_f32(const float* logits, const float* fc2w, int P, int nc, float* pvec, float* dens,
                              mlsp_stream_t stream);
int mlsp_density_tail_bwd_f32(const float* pvec, const float* fc2w, const float* dpvec, const float* ddens, int P, int nc,
                              float* dlogits, mlsp_stream_t stream);

/* densityloss (MLSP/mlsp.py:430-454): out = {kl, mae, sum mask}; mask nullable */
int mlsp_density_loss_fwd_f32(const float* pvec, const float* dens, const float* target_vec, const float* target,
                              const float* mask, int P, int nc, float density_weight, float* out, void* ws, size_t ws_bytes,
                              mlsp_stream_t stream);
int mlsp_density_loss_bwd_f32(const float* pvec, const float* dens, const float* target_vec, const float* target,
                              const float* mask, int P, int nc, float density_weight, const float* fwd_out,
                              const float* grad_kl, const float* grad_mae, float* dpvec, float* ddens, mlsp_stream_t stream);

/* Index-matched losses on the deformed region (def_loss.hip).  N <= 4096 (MLSP_ERR_UNSUPPORTED otherwise); indices are int64 [B][N]
 * as torch.min returns them; an index outside [0, N) is never dereferenced (its row contributes zero).
 * mask [B][3][N] (row 0 is used); defpart = args.Density_normal_defpart: row weight w = m if set, 26 m + 1 otherwise.
 *
 * findindexs / findneareat_index (MLSP/mlsp.py:184-220): pred [B][N][3], gold [B][3][N];
 * index1[b][i] = argmin_j |pred_bi - gold_bj|^2 + pen_bj, index2[b][j] = argmin_i |gold_bj - pred_bi|^2 + pen_bi, pen = 100 where
 * mask == 0 and 0 where it is 1; distance as torch.norm(...)**2 in fp32; ties go to the lowest index. */
int mlsp_def_nearest_index_f32(const float* pred, const float* gold, const float* mask, int B, int N, int64_t* index1, int64_t* index2,
                               mlsp_stream_t stream);

/* calc_def_normal_loss (MLSP/mlsp.py:289-329): pred, labels [B][N][3];
 * out[0] = -weight/B sum_b (sum_i w_bi |n(pred_bi).n(lab_b,idx1)| + sum_j w_bj |n(pred_b,idx2).n(lab_bj)|) / sum_i w_bi,
 * out[1 + b] = sum_i w_bi (out has 1 + B floats, kept for the backward).  ws: 16 B bytes.  The backward writes dpred [B][N][3]
 * (no gradient to the labels); its scatter through index2 runs in a fixed order (deterministic). */
int mlsp_def_normal_loss_fwd_f32(const float* pred, const float* labels, const float* mask, const int64_t* index1, const int64_t* index2,
                                 int B, int N, int defpart, float weight, float* out, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_def_normal_loss_bwd_f32(const float* pred, const float* labels, const float* mask, const int64_t* index1, const int64_t* index2,
                                 int B, int N, int defpart, float weight, const float* fwd_out, const float* grad_loss, float* dpred,
                                 mlsp_stream_t stream);

/* deform_densityloss (MLSP/mlsp.py:370-427): pvec [B*N][nc] and dens [B*N] (logits['density'], logits['density_mse']), label_vec
 * [B*N][nc], label_val [B*N].  out = {kl + kl1, mae + mae1, sum w}: the two densityloss (:430-454) evaluations, labels gathered
 * through index1 against the predictions, then predictions gathered through index2 as the target of the labels.  ws: 6 KiB.
 * The backward writes dpvec [B*N][nc] and ddens [B*N] (grad_kl / grad_mae nullable = 0), scattered deterministically. */
int mlsp_def_density_loss_fwd_f32(const float* pvec, const float* dens, const float* label_vec, const float* label_val, const float* mask,
                                  const int64_t* index1, const int64_t* index2, int B, int N, int nc, int defpart, float density_weight,
                                  float* out, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_def_density_loss_bwd_f32(const float* pvec, const float* dens, const float* label_vec, const float* label_val, const float* mask,
                                  const int64_t* index1, const int64_t* index2, int B, int N, int nc, int defpart, float density_weight,
                                  const float* fwd_out, const float* grad_kl, const float* grad_mae, float* dpvec, float* ddens,
                                  mlsp_stream_t stream);

/* the row gathers of calc_def_density_loss (MLSP/mlsp.py:346-348, :359-361): out[b][j][:] = x[b][index[b][j]][:], rows of W 32-bit
 * words (bits copied, so int64 class labels gather as W = 2); the backward dx[b][i][:] = sum over j with index[b][j] == i of
 * dout[b][j][:] (C floats per row) in ascending j -- deterministic. */
int mlsp_gather_rows_u32(const void* x, const int64_t* index, int B, int N, int W, void* out, mlsp_stream_t stream);
int mlsp_gather_rows_bwd_f32(const float* dout, const int64_t* index, int B, int N, int C, float* dx, mlsp_stream_t stream);

/* plain fp32 GEMM on the matrix cores (exposed for tests and the 3x3 input transform):
 * C[M][N] = opA(A) opB(B) + bias;  ta/tb as in gemm.hip */
int mlsp_gemm_f32(int ta, int tb, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                  const float* bias, int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);

/* Label generators of the target branch (python-pcl in the reference, PARITY UNPINNED -- see labels.hip):
 * radius neighbour count behind cal_density (MLSP/mlsp.py:240-272; count excludes cloud index 0, capped at max_nn) and
 * k-neighbourhood PCA normals behind kSearchNormalEstimation (PointDA/trainer.py:173-188; idx from mlsp_knn_f32, self
 * included; oriented towards the origin).  x [B][N] rows of >= 3 floats, row pitch ldx. */
int mlsp_radius_count_f32(const float* x, int ldx, int B, int N, float radius, int max_nn, int32_t* count, mlsp_stream_t stream);
int mlsp_knn_normals_f32(const float* x, int ldx, const int32_t* idx, int B, int N, int k, float* normals, mlsp_stream_t stream);

/* PointNet++ set-abstraction front end (BASELINE.json configs[3]).  The reference states the semantics in
 * PointDA/hengshuang_transformer/pointnet_util.py only: farthest_point_sample :53-73 (start index supplied by the caller --
 * the reference draws it with torch.randint :65), query_ball_point :76-96 (first nsample indices with !(d2 > r2) in index
 * order, padded with the first), sample_and_group :99-136 (rows [xyz_j - new_xyz_i | feat_j], edge-major (b, i, s)).
 * xyz [B][N] rows of >= 3 floats (pitch ldx); new_xyz [B][S] rows (pitch ldq); feat [B*N][D] or NULL when D == 0;
 * idx / fps_idx are int32 local to their cloud.  mlsp_group_reverse builds the reverse index of idx [B][S][ns] over the
 * N source points (same format as mlsp_knn_reverse) for the deterministic backward of the grouping. */
/* kNN of query points among DIFFERENT reference points: `square_distance` + argsort()[:, :, :k] (pointnet_util.py:26-38,116-118 knn=True
 * grouping, :237-239 Msg, :287-289 the 3-NN of feature propagation; the KNN calls of PointDA/model_utils.py:175,188 have this shape).
 * d = sum_c (q_c - r_c)^2 in fp32 -- the reference's return statement (pointnet_util.py:36), c ascending over the C <= 8 coordinates,
 * ((dx*dx + dy*dy) + dz*dz) + ..., no contraction: never negative, exactly 0 at coincident points -- ascending, ties -> lower reference index.
 * ref [B][Nr] rows (pitch ldr), qry [B][Nq] rows (pitch ldq) -> idx [B][Nq][k] (local to the cloud), dist [B][Nq][k] (nullable). k <= 64.
 * Index contract: every returned index lies in [0, Nr), whatever the coordinates hold (k <= Nr is required).  A distance that is not
 * finite (a NaN coordinate in the query or the reference, a squared norm that overflows) counts as +inf; +inf candidates fill the slots
 * that no finite candidate took, lowest reference index first, and dist reports +inf for them.  The consumers of idx gather without a
 * range check. */
int mlsp_knn_query_f32(const float* ref, int ldr, int Nr, const float* qry, int ldq, int Nq, int B, int C, int k, int32_t* idx, float* dist,
                       mlsp_stream_t stream);
/* PointNetFeaturePropagation interpolation (pointnet_util.py:287-294): out [B][N][D] = inverse-distance weighted mean of the features
 * feat [B][S][D] of the three nearest sampled points (idx, dist [B][N][3] from mlsp_knn_query_f32); backward over the reverse index of idx
 * (mlsp_group_reverse(idx, B, N, S, 3, ...)): dfeat [B][S][D], deterministic order. */
int mlsp_interp3_fwd_f32(const float* feat, const int32_t* idx, const float* dist, int B, int N, int S, int D, float* out, mlsp_stream_t stream);
int mlsp_interp3_bwd_f32(const float* dout, const float* dist, const int32_t* rev_off, const int32_t* rev_ent, int B, int N, int S, int D,
                         float* dfeat, mlsp_stream_t stream);
int mlsp_fps_f32(const float* xyz, int ldx, int B, int N, int S, const int32_t* start, int32_t* fps_idx, mlsp_stream_t stream);
/* Which kernel mlsp_fps_f32 runs a cloud of N points on (host arithmetic only, no launch): 2 = the four-wave DPP kernel (64 <= N <= 2048),
 * 1 = the 1024-thread kernel (every other N up to 8192), 0 = no kernel (N <= 0 or N > 8192: mlsp_fps_f32 returns MLSP_ERR_ARG). */
int mlsp_fps_plan(int N);
/* (a query without a hit inside the radius -- the reference indexes out of range there -- gets 0 in every slot) */
int mlsp_ball_query_f32(const float* xyz, int ldx, const float* new_xyz, int ldq, int B, int N, int S, float radius_sq, int nsample,
                        int32_t* idx, mlsp_stream_t stream);
int mlsp_group_reverse(const int32_t* idx, int B, int S, int N, int ns, int32_t* rev_off, int32_t* rev_ent, mlsp_stream_t stream);
int mlsp_sa_group_fwd_f32(const float* xyz, int ldx, const float* feat, int D, const float* new_xyz, int ldq, const int32_t* idx, int B,
                          int N, int S, int ns, float* G, mlsp_stream_t stream);
/* dfeat [B][N][D] = the sum, over the groups a point sits in, of columns [col, col + D) of the grouped-row gradient dG (row pitch ldg):
 * col = 3 for the feature columns, col = 0 / D = 3 for the coordinate columns (d xyz of `grouped_xyz - new_xyz`, pointnet_util.py:122-124). */
int mlsp_sa_group_bwd_f32(const float* dG, int ldg, int col, int D, const int32_t* rev_off, const int32_t* rev_ent, int B, int N, int S, int ns,
                          float* dfeat, mlsp_stream_t stream);

/* Linear + BatchNorm + activation + max over the k consecutive rows of every group, fused (pointnet_util.py:188-195: the last conv of a
 * set-abstraction MLP and `torch.max(new_points, 2)[0]`; also sample_and_group_all with k = N <= 255).  X [M][Cin] edge rows, M = G*k.
 * fwd: Y [M][Cout] pre-BN output (kept for the backward), out [G][Cout] = max_s act(BN(y)), ysel [G][Cout] the selected pre-BN value
 * (max for scale >= 0, min otherwise), argk [G][Cout] uint8 its first slot, bn_save [4][Cout].  The activated tensor is never written.
 * bwd: dOut [G][Cout] -> dX (nullable) [M][Cin], dW [Cout][Cin], dbias (nullable), dgamma, dbeta; the BatchNorm sums come from the
 * G*Cout selected entries, the gradient of the activated tensor is never materialised.  k <= 255, Cout % 4 == 0, 256 % (Cout/4) == 0. */
int mlsp_pointmlp_segmax_fwd_f32(const float* X, int ldx, int M, int Cin, const float* W, int ldw, int Cout, const float* bias,
                                 const float* gamma, const float* beta, float* run_mean, float* run_var, float momentum, float eps,
                                 int training, int act, float slope, int k, float* Y, float* out, float* ysel, uint8_t* argk, float* bn_save,
                                 int precision, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_pointmlp_segmax_bwd_f32(const float* dOut, const float* X, int ldx, int M, int Cin, const float* W, int ldw, int Cout, const float* Y,
                                 const float* ysel, const uint8_t* argk, const float* bn_save, int training, int act, float slope, int k,
                                 float* dX, int lddx, float* dW, float* dbias, float* dgamma, float* dbeta, int precision, void* ws, size_t ws_bytes,
                                 mlsp_stream_t stream);

/* Folded first layer of a set-abstraction MLP (pointnet_util.py:120-129 grouping + :185-190 first Conv2d + BatchNorm2d + ReLU): the
 * conv over the edge rows [x_j - c_i | f_j] equals u_j - w_i with u [B*N][C] = [x | f] W^T + b per source point and w [B*S][C] = c Wx^T
 * per centre (two per-point GEMMs the caller runs with mlsp_pointmlp_fwd_f32 / mlsp_gemm_f32); neither the grouped tensor nor the
 * pre-BN output is materialised.  idx [B][S][ns] int32 (indices local to the cloud, as mlsp_ball_query_f32 / mlsp_knn_query_f32
 * return them).  fwd: BatchNorm over the E = B*S*ns edges (training: batch statistics, running buffers updated; eval: running
 * buffers), Z [E][C] = relu(scale * (u_j - w_i) + shift), bn_save [4][C] = scale | shift | mean | invstd.
 * bwd: dZ [E][C] -> du [B*N][C], dw [B*S][C] (closed-form BN backward; du over the reverse index of idx from
 * mlsp_group_reverse(idx, B, S, N, ns, ...): fixed summation order), dgamma, dbeta [C].
 * C in {16, 32, 64, 128, 256}, ns <= 256; MLSP_ERR_UNSUPPORTED otherwise (the caller keeps the grouped path). */
int mlsp_sa_fold_fwd_f32(const float* u, const float* w, const int32_t* idx, int B, int N, int S, int ns, int C, const float* gamma,
                         const float* beta, float* run_mean, float* run_var, float momentum, float eps, int training, float* Z,
                         float* bn_save, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_sa_fold_bwd_f32(const float* dZ, const float* u, const float* w, const int32_t* idx, const int32_t* rev_off, const int32_t* rev_ent,
                         const int32_t* rev_cnt, const int32_t* pad_cnt, int B, int N, int S, int ns, int C, const float* bn_save, int training,
                         float* du, float* dw, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, mlsp_stream_t stream);
/* Reverse index of padded groups WITHOUT their padding slots (ball-query groups end in copies of their first hit: the padding slots of a
 * group are its TRAILING run of slots s > 0 with idx[i][s] == idx[i][0]; a repeat of slot 0 further up a row is an ordinary slot, so any
 * idx is handled, not only ball-query output): rev_off [B*N+1] list starts, rev_cnt [B*N] list lengths (the lists of a cloud no longer fill its S*ns entries), rev_ent as
 * mlsp_group_reverse, pad_cnt [B*S] padding slots per group.  mlsp_sa_fold_bwd_f32 takes rev_cnt / pad_cnt (both or neither, NULL = the
 * full index of mlsp_group_reverse) and adds a group's identical padding rows as a multiple of one row.  The compact form rests on a
 * premise the caller must meet: every padding row of a group carries the same dZ as the group's LAST slot (the row that is read for all
 * of them), as it does behind the layer's own forward; for any other dZ pass the full index. */
int mlsp_group_reverse_compact(const int32_t* idx, int B, int S, int N, int ns, int32_t* rev_off, int32_t* rev_cnt, int32_t* rev_ent,
                               int32_t* pad_cnt, mlsp_stream_t stream);

/* Input corruption.  mlsp_region_assign_f32: utils/pc_utils.py:33-73 assign_region_to_point on X [B][C][N]
 * (channel-major as the trainer holds it); thr[n+1] = fp32 voxel edges, clip = fp32(0.99999999); regions int32 [B][N].
 * mlsp_deform_regions_f32: MLSP/mlsp.py:10-51 deform_input, DefRec_dist == 'volume_based_voxels': per cloud the first
 * `groups` regions of `order` (np.random.permutation(n^3) in the reference, :27) holding >= min_pts points are replaced by
 * lookup[region] + noise (noise [B][3][N], already scaled by sqrt(0.001): pc_utils.draw_from_gaussian :114-122);
 * X is updated in place, mask [B][C][N] receives 1 on the first three channels of the replaced points, 0 elsewhere. */
int mlsp_region_assign_f32(const float* X, int B, int C, int N, const float* thr, int n, float clip, int32_t* regions, mlsp_stream_t stream);
int mlsp_deform_regions_f32(float* X, int B, int C, int N, const int32_t* regions, const int32_t* order, int nreg, const float* lookup,
                            const float* noise, int min_pts, int groups, float* mask, mlsp_stream_t stream);
/* Input transform (PointDA/Models.py:113 `x = torch.matmul(transformd_x0, x)`, PointSegDA/Models.py:218): out [B*N][3], out[p] = T[b] x[p] for the
 * points of cloud b; x [B*N][3] point-major, T [B][3][3].  Backward: dx (nullable) [B*N][3] and dT [B][3][3] (fixed reduction order). */
int mlsp_transform3_fwd_f32(const float* x, const float* T, int B, int N, float* out, mlsp_stream_t stream);
int mlsp_transform3_bwd_f32(const float* x, const float* T, const float* dout, int B, int N, float* dx, float* dT, mlsp_stream_t stream);

/* Two 1x1 convolutions with nothing in between (PointSegDA/Models.py:176-178, :180-182 `x = self.conv2(self.conv1(x))`) are ONE linear map:
 * W [Co][Ci] = Wb Wa, b [Co] = Wb ba + bb with Wa [Cm][Ci], ba [Cm], Wb [Co][Cm], bb [Co] (row-major, fmaf chains over m ascending).
 * Backward: dWa [Cm][Ci] = Wb^T dW, dba [Cm] = Wb^T db, dWb [Co][Cm] = dW Wa^T + db ba^T (the gradient of bb is db itself).
 * Ci, Cm, Co <= 1024. */
int mlsp_compose_linear_fwd_f32(const float* Wa, const float* ba, const float* Wb, const float* bb, int Cm, int Ci, int Co, float* W, float* b,
                                mlsp_stream_t stream);
int mlsp_compose_linear_bwd_f32(const float* dW, const float* db, const float* Wa, const float* ba, const float* Wb, int Cm, int Ci, int Co,
                                float* dWa, float* dba, float* dWb, mlsp_stream_t stream);

/* deform_input(..., 'volume_based_radius') = pc_utils.collapse_to_point (MLSP/mlsp.py:33-36, utils/pc_utils.py:76-111): per cloud one
 * point with >= min_pts points within sqrt(radius2) is picked (uniformly by u[b] in [0,1) among the candidates in index order, or
 * choice[b] >= 0 pins it) and all points within that radius of it become centre + noise (noise [B][3][N], already scaled by the
 * Gaussian's std); mask [B][3][N] marks them; chosen[b] = the picked index or -1 when the cloud has no candidate (left untouched).
 * X [B][3][N] is updated in place. */
int mlsp_collapse_to_point_f32(float* X, int B, int N, const int32_t* choice, const float* u, const float* noise, float radius2,
                               int min_pts, float* mask, int32_t* chosen, mlsp_stream_t stream);

/* MLSP/mlsp.py:54-89 scan_input / p_scan: X [B][N][C] point-major; R [B][9] float64 row-major rotation of every cloud
 * (rotate_point_cloud_3d :91-112, drawn on the host); pixel = int(2 / pixel_size).  Xs [B][N][C] keeps only the visible points,
 * mask [B][N][C] is 0 on their first three channels and 1 elsewhere. */
int mlsp_scan_select_f32(const float* X, int B, int N, int C, const double* R, int pixel, float* Xs, float* mask, mlsp_stream_t stream);

/* (ABI v7's process-wide mlsp_set_gemm_precision is gone: see `precision` in the conventions above.) */

/* Measurement aid (bench.py `roofline`): while armed, every gemm_f32_kernel launch is bracketed by two HIP
 * events on its launch stream.  mlsp_profile_end synchronises those events and fills
 * out[4] = {total ms in the kernel, launches, sum of algorithmic 2*M*N*K, sum of the A + B + C bytes}.  Not for production steps. */
int mlsp_profile_begin(void);
int mlsp_profile_end(double* out);
/* Per kernel class of the same bracket (call after mlsp_profile_end): out [MLSP_PROF_CLASSES][3] = {ms, launches, algorithmic work}.
 * Classes: 0 GEMM family (FLOP) | 1 kNN C <= 4 incl. its row norms (compulsory bytes: (C + k) * 4 per point) | 2 kNN C = 64 |
 * 3 kNN C = 128 (FLOP: 2 N C per point) | 4 EdgeConv neighbour gather-reduce (compulsory bytes) | 5 T-Net per-edge stage forward |
 * 6 its backward (FLOP of the 64 -> 128 per-edge contraction: 2 resp. 4 * E * 64 * 128) | 7 the launches of class 0 that ran on the
 * bf16-split kernel (mode 2; algorithmic FLOP, each executed as six bf16 MFMA products). */
#define MLSP_PROF_CLASSES 8
int mlsp_profile_classes(double* out, int ncls);
/* out [4][4]: {ms, launches, algorithmic FLOP, algorithmic bytes} of the bracket's gemm_split_kernel launches by kind (forward, dgrad, wgrad);
 * row 3 (ABI v13): those of all kinds that ran on the two-piece f16 products (MLSP_PREC_F16X3). */
int mlsp_profile_split_kinds(double* out);
/* The bracket's GEMM-family launches one by one, in launch order (call after mlsp_profile_end): out [max_rows][MLSP_PROF_LAUNCH_COLS] =
 * {M, N, K, ta, tb, K splits, tile rows, epilogue bits, split (0 | 1 = bf16 pieces | 2 = f16 pieces), extra bits, kernel family
 * (0 FOLD64 | 1 N64 | 2 F32_EDGE | 3 F32 | 4 BF16 | 5 SPLIT), grid x, grid y, slab reducer (0-2 VEC 8 / 4 / 1 | 3 WAVE | 4 SCALAR |
 * 5-7 UNFOLD 8 / 4 / 1; -1: one pass)}.  Returns the number of launches recorded (at most max_rows rows are written) or a negative
 * MLSP_ERR_*.  What the tests read to assert the kernel a shape reached; it changes no kernel choice.  (Symbol added under ABI v14:
 * a v14 library built before it lacks it, and the Python binding says so when it loads one.) */
#define MLSP_PROF_LAUNCH_COLS 14
int mlsp_profile_launches(int32_t* out, int max_rows);

/* Adam step (PointDA/trainer.py:258-259, stepped at :571) over flat parameter / exp_avg / exp_avg_sq buffers P / M / V in ONE launch:
 * segment s covers elements [off[s], off[s] + numel[s]) of the three buffers (buffers 16-byte aligned; off % 4 == 0 takes the 16-byte path) and reads its
 * gradient where autograd left it (grads[s], contiguous fp32, device).  off / numel / grads are HOST arrays.  step >= 1 numbers this
 * update (bias corrections 1 - beta^step); step_out (nullable, device float) receives it.  The element-wise arithmetic restates
 * torch's fused Adam (ATen/native/cuda/fused_adam_utils.cuh, ADAM_MODE::ORIGINAL: weight decay added to the gradient) type by type.
 * tile_amax (nullable; ABI v13): one float per 2048-element tile -- tiles numbered segment by segment in the order given, ceil(numel[s] /
 * 2048) per segment -- receives the largest magnitude of the tile's UPDATED parameters: a free bound for the GEMMs that read the
 * parameters next (mlsp_bound_t: partials = tile_amax + first tile of the weight, n = its tiles). */
int mlsp_adam_flat_f32(float* P, float* M, float* V, const uint32_t* off, const uint32_t* numel, const float* const* grads, int nseg, double lr,
                       double beta1, double beta2, double weight_decay, double eps, int64_t step, float* step_out, float* tile_amax,
                       mlsp_stream_t stream);
/* SGD step (torch.optim.SGD: PointDA/trainer.py:258-259, PointDA/train_spst.py, PointSegDA/trainer.py:212-214 with --optimizer SGD) over the flat
 * parameter buffer P and momentum buffer B in ONE launch; segments, gradients, tiles and tile_amax as mlsp_adam_flat_f32.  B (16-byte
 * aligned) may be NULL when momentum == 0.  first != 0: B is initialised with the (decayed) gradient instead of updated -- torch's first step.
 * The element-wise arithmetic restates torch's default multi-tensor SGD (torch/optim/sgd.py _multi_tensor_sgd) type by type: maximize
 * negates the gradient, then g += (float)weight_decay * p, buf = buf * (float)momentum + (float)(1 - dampening) * g, g = nesterov ? g +
 * (float)momentum * buf : buf, p += (float)(-lr) * g, every `a + alpha * b` one fma as in torch's ROCm build. */
int mlsp_sgd_flat_f32(float* P, float* B, const uint32_t* off, const uint32_t* numel, const float* const* grads, int nseg, double lr,
                      double momentum, double dampening, double weight_decay, int nesterov, int maximize, int first, float* tile_amax,
                      mlsp_stream_t stream);

/* The same two steps for a model split into parameter groups (at most MLSP_FLAT_MAX_GROUPS: "no weight decay on BatchNorm and biases",
 * per-group learning rates), still ONE launch: seg_group[s] (host array, nullable = all 0) names the group of segment s, groups[] (host
 * array, ngroups entries) holds every group's hyperparameters, and each workgroup reads those of the segment that owns its tile.  The
 * segments may come in any order of groups: tiles and tile_amax are numbered segment by segment as above.  Symbols added under ABI v13.
 * Adam: a group's step >= 1 numbers this update for its parameters and goes to its step_out (nullable, device float).  decoupled != 0 is
 * AdamW (fused_adam_utils.cuh ADAM_MODE::ADAMW): param -= lr * weight_decay * param in double before the moments, the gradient untouched.
 * SGD: B may be NULL only when every group has momentum == 0; first is per group.
 * MLSP_ERR_ARG before any launch: ngroups outside [1, 8], a seg_group entry outside [0, ngroups), a group with step < 1, a NULL or
 * misaligned flat buffer, momentum != 0 in some group while B is NULL, a NULL gradient or an empty segment.
 * mlsp_adam_flat_f32 / mlsp_sgd_flat_f32 are the one-group forms of these. */
#define MLSP_FLAT_MAX_GROUPS 8
typedef struct mlsp_adam_group { double lr, beta1, beta2, weight_decay, eps; int64_t step; int32_t decoupled; float* step_out; } mlsp_adam_group_t;
typedef struct mlsp_sgd_group { double lr, momentum, dampening, weight_decay; int32_t nesterov, maximize, first; } mlsp_sgd_group_t;
int mlsp_adam_flat_groups_f32(float* P, float* M, float* V, const uint32_t* off, const uint32_t* numel, const float* const* grads,
                              const uint8_t* seg_group, int nseg, const mlsp_adam_group_t* groups, int ngroups, float* tile_amax,
                              mlsp_stream_t stream);
int mlsp_sgd_flat_groups_f32(float* P, float* B, const uint32_t* off, const uint32_t* numel, const float* const* grads, const uint8_t* seg_group,
                             int nseg, const mlsp_sgd_group_t* groups, int ngroups, float* tile_amax, mlsp_stream_t stream);

/* The edge stages of the vector-attention block (PointDA/hengshuang_transformer/transformer.py:28-44) between its GEMMs (csrc/vecattn.hip).
 * P = B N points, k slots per point (1 <= k <= 64), E = P k edges, e = (i, s), j = idx[i][s] (int32 [B][N][k], local to the cloud; an
 * entry may repeat inside a row).  Every [E][d] / [P][d] matrix is fp32, channels contiguous; d % 4 == 0, pointers and row pitches
 * 16-byte aligned (xyz: any pitch ldx >= 3) -- anything else returns MLSP_ERR_UNSUPPORTED.  No entry reaches a matrix core.
 * delta_fwd (transformer.py:37, first layer of fc_delta): H1[e][c] = relu(sum_a Wd1[c][a] (xyz_i[a] - xyz_j[a]) + bd1[c]), Wd1 [d][3]. */
int mlsp_vecattn_delta_fwd_f32(const float* xyz, int ldx, const int32_t* idx, const float* Wd1, const float* bd1, int B, int N, int k, int d,
                               float* H1, mlsp_stream_t stream);
/* transformer.py:37 backward: dWd1 [d][3] and dbd1 [d] from dH1 and H1 (mask H1 > 0), summed in a fixed order through the workspace.
 * No gradient to xyz. */
int mlsp_vecattn_delta_bwd_f32(const float* dH1, const float* H1, const float* xyz, int ldx, const int32_t* idx, int B, int N, int k, int d,
                               float* dWd1, float* dbd1, void* ws, size_t ws_bytes, mlsp_stream_t stream);
/* transformer.py:39, the input of fc_gamma: T[e] = q_i - kk_j + pos[e]; q / kk [P][d] with row pitches ldq / ldk. */
int mlsp_vecattn_mix_fwd_f32(const float* q, int ldq, const float* kk, int ldk, const float* pos, const int32_t* idx, int B, int N, int k, int d,
                             float* T, mlsp_stream_t stream);
/* transformer.py:39 backward: dq_i = sum_s dT[i][s].  (dpos = dT; dkk_j = -(reverse-index sum of dT): mlsp_group_reverse +
 * mlsp_sa_group_bwd_f32.) */
int mlsp_vecattn_mix_bwd_f32(const float* dT, int B, int N, int k, int d, float* dq, mlsp_stream_t stream);
/* transformer.py:40-42: attn [E][d] = softmax over the k slots of A / sqrt(d) per channel (maximum subtracted), res [P][d] =
 * sum_s attn[i][s] * (v_j + pos[i][s]); v [P][d] with row pitch ldv. */
int mlsp_vecattn_aggregate_fwd_f32(const float* A, const float* v, int ldv, const float* pos, const int32_t* idx, int B, int N, int k, int d,
                                   float* attn, float* res, mlsp_stream_t stream);
/* transformer.py:40-42 backward from dres: dVP[e] = attn[e] * dres_i (the gradient of v_j + pos[e]: add to dpos, reverse-index sum -> dv)
 * and dA[e] = attn[e] * (g[e] - sum_s attn[i][s] g[i][s]) / sqrt(d), g[e] = dres_i * (v_j + pos[e]).  attn itself takes no gradient. */
int mlsp_vecattn_aggregate_bwd_f32(const float* dres, const float* attn, const float* v, int ldv, const float* pos, const int32_t* idx, int B,
                                   int N, int k, int d, float* dVP, float* dA, mlsp_stream_t stream);
/* transformer.py:39, the ReLU inside fc_gamma on [rows][d] (the GEMM family activates only behind a BatchNorm): y = max(x, 0), y may be x;
 * backward dx = dy where y > 0. */
int mlsp_vecattn_relu_fwd_f32(const float* x, int64_t rows, int d, float* y, mlsp_stream_t stream);
int mlsp_vecattn_relu_bwd_f32(const float* dy, const float* y, int64_t rows, int d, float* dx, mlsp_stream_t stream);

/* What the Point-BERT transformer encoder (PointDA/model_utils.py:201-289) runs between its GEMMs (csrc/attn.hip): the multi-head attention
 * core, LayerNorm and GELU.  fp32 throughout (no product mode); every pointer and row pitch 16-byte aligned, channel counts multiples of 4;
 * anything outside the limits returns MLSP_ERR_UNSUPPORTED and launches nothing.  No atomics: results are bit-identical run to run.
 *
 * Attention core.  qkv [B L][ld] is the qkv GEMM's output as it stands: with d = H dh, the q, k and v of head h are the column slices at
 * h dh, d + h dh and 2 d + h dh (ld >= 3 d).  out [B L][d] (head-interleaved: the reference's transpose(1, 2).reshape) = softmax(scale q k^T) v
 * per (cloud, head); lse [B][H][L] = row maximum + log(row sum) of the scaled logits.  One launch; nothing of size L^2 touches memory.
 * Limits: dh % 4 == 0, dh <= 128, L <= 512 and L dh <= 16384 (two [L][dh] fp32 arrays of a head stay in LDS). */
int mlsp_mhsa_fwd_f32(const float* qkv, int ld, int B, int L, int H, int dh, float scale, float* out, float* lse, mlsp_stream_t stream);
/* dqkv [B L][ldd] in qkv's layout (every element of its first 3 d columns is written) from dout [B L][d] and the forward's qkv and lse:
 * P = exp(scale q k^T - lse) and dP = dout v^T are recomputed, delta_i = sum_j P_ij dP_ij / sum_j P_ij (= dout_i . out_i in exact arithmetic; `out`
 * itself is not read), dS = P (dP - delta), dq = scale dS k, dk = scale dS^T q, dv = P^T dout.  One launch; same limits. */
int mlsp_mhsa_bwd_f32(const float* qkv, int ld, const float* lse, const float* dout, int B, int L, int H, int dh, float scale, float* dqkv, int ldd,
                      mlsp_stream_t stream);
/* u = x + sample_scale[row / rows_per_sample] * add (add NULL: u = x and `u` is not written; sample_scale NULL: 1), y = LayerNorm(u) * gamma
 * + beta over the d channels of each of `rows` contiguous rows (biased variance), mean / rstd [rows] saved for the backward.  gamma NULL:
 * only u is written (the residual add at a block's exit; add and u required).  sample_scale carries DropPath: mask_b / keep_prob. */
int mlsp_layernorm_fwd_f32(const float* x, const float* add, const float* sample_scale, int rows_per_sample, const float* gamma, const float* beta,
                           int64_t rows, int d, float eps, float* u, float* y, float* mean, float* rstd, mlsp_stream_t stream);
/* dx = (gradient of y through the normalisation, from the saved u, mean, rstd) + du (du nullable: the gradient that reached u directly);
 * dadd (nullable) = sample_scale * dx; dgamma / dbeta [d]: per-workgroup partials in the workspace summed in a fixed order in fp64.
 * dy NULL is the backward of the gamma == NULL forward: dadd = sample_scale * du and nothing else is written. */
int mlsp_layernorm_bwd_f32(const float* dy, const float* du, const float* u, const float* sample_scale, int rows_per_sample, const float* gamma,
                           const float* mean, const float* rstd, int64_t rows, int d, float* dx, float* dadd, float* dgamma, float* dbeta,
                           void* ws, size_t ws_bytes, mlsp_stream_t stream);
/* y = x Phi(x), the erf form of GELU (nn.GELU()'s default), on [rows][d];  dx = dy (Phi(x) + x phi(x)) from the saved x. */
int mlsp_gelu_fwd_f32(const float* x, int64_t rows, int d, float* y, mlsp_stream_t stream);
int mlsp_gelu_bwd_f32(const float* dy, const float* x, int64_t rows, int d, float* dx, mlsp_stream_t stream);

/* The edge stage of DGCNN_Propagation (PointDA/Models.py:327-363: get_graph_feature, layer1 / layer2 = Conv2d(1x1, no bias) + GroupNorm +
 * LeakyReLU, max over the k neighbours) behind its FOLDED convolution.  With the conv weight W = [Wa | Wb] over the edge input
 * [f_j - f_i ; f_i] (:347) the pre-norm value of edge (i, s) is y(i, s, c) = u[j][c] + w[i][c], j = idx[i][s]: u [B*Nk][C] = f_k Wa^T per
 * source point (row pitch ldu), w [B*Nq][C] = f_q (Wb - Wa)^T per query point (row pitch ldw) -- two per-point GEMMs the caller runs
 * (mlsp_pointmlp_fwd_f32).  idx [B][Nq][k] int32, local to the cloud, as mlsp_knn_query_f32 returns it (an index outside [0, Nk) is read
 * as 0; an entry may repeat inside a row).  Never materialised, in either direction: the [B][2 Cin][Nq][k] edge tensor, the [B][C][Nq][k]
 * conv output, its normalised / activated copies and their gradients.
 * fwd: stats [B][groups][2] = mean and 1 / sqrt(biased variance + eps) of y over the (C / groups) Nq k values of a (cloud, group) (fp64
 * sums, per-workgroup partials in the workspace added in ascending order);  out [B*Nq][C] = max_s lrelu((y - mean) rstd gamma[c] + beta[c]);
 * argk [B*Nq][C] uint8 = the slot that attains it: the first maximum of y where gamma[c] rstd >= 0, the first minimum otherwise -- in [0, k)
 * for every input (a NaN in y makes the group's statistics, hence its outputs, NaN).
 * bwd: from dOut [B*Nq][C] and the saved u, w, idx, argk, stats and the reverse index of idx (mlsp_group_reverse(idx, B, Nq, Nk, k, ...)):
 * dz = dOut lrelu'(.) at the selected slot, dy(i, s, c) = rstd (gamma[c] dz [s == argk] - A - yhat(i, s, c) Bm) with A / Bm the group means
 * of gamma dz / gamma dz yhat;  dw [B*Nq][C] = sum_s dy (ascending s), du [B*Nk][C] = sum of dy over the edges that name the row
 * (reverse-index order; exactly 0 for a row no edge names), dgamma / dbeta [C] = sum dz yhat_sel / sum dz (fp32 per-workgroup partials,
 * added in fp64 in ascending order).  No atomics.
 * Limits: C % (4 groups) == 0, groups <= 256, 1 <= k <= 64, Nk, Nq <= 2^22, 16-byte-aligned pointers and row pitches (ldu, ldw % 4 == 0)
 * -- anything else returns MLSP_ERR_UNSUPPORTED and launches nothing.  No entry reaches a matrix core.
 * ws: at least mlsp_gn_edge_workspace_bytes(...) bytes (0 for a shape outside the limits). */
size_t mlsp_gn_edge_workspace_bytes(int B, int Nk, int Nq, int k, int C, int groups);
int mlsp_gn_edge_fwd_f32(const float* u, int ldu, const float* w, int ldw, const int32_t* idx, const float* gamma, const float* beta, int B, int Nk,
                         int Nq, int k, int C, int groups, float eps, float slope, float* out, uint8_t* argk, float* stats, void* ws,
                         size_t ws_bytes, mlsp_stream_t stream);
int mlsp_gn_edge_bwd_f32(const float* dOut, const float* u, int ldu, const float* w, int ldw, const int32_t* idx, const uint8_t* argk,
                         const float* stats, const int32_t* rev_off, const int32_t* rev_ent, const float* gamma, const float* beta, int B, int Nk,
                         int Nq, int k, int C, int groups, float slope, float* du, float* dw, float* dgamma, float* dbeta, void* ws,
                         size_t ws_bytes, mlsp_stream_t stream);

/* The two stages of the Point-BERT PointTransformer (PointDA/Models.py:365-531) that the GEMM family serves badly (token.hip).  fp32; no
 * atomics: results are bit-identical run to run; anything outside the limits returns MLSP_ERR_UNSUPPORTED and launches nothing.
 *
 * Thin-input layer: H [M][C] = act(BN?(X W^T + b)), X [M][Cin] (row pitch ldx >= Cin, Cin <= 8), W [C][Cin] contiguous, C % 4 == 0,
 * C <= 4096, act in {0 none, 1 relu, 3 gelu (erf form)}; H and every per-channel vector 16-byte aligned.  bias nullable.
 * gamma == NULL (then beta == NULL): no BatchNorm.  Otherwise training != 0 normalises with the batch statistics, which come from the
 * input's first and second moments (mean_c = w_c mu + b_c, var_c = w_c^T Sigma w_c; fp64 sums, fixed order) -- no pre-BN tensor exists;
 * M < 2 is MLSP_ERR_ARG.  xmom [72] doubles = mu[8] | Sigma[8][8] is written for the backward; run_mean / run_var (nullable) are updated
 * as torch does (unbiased variance, `momentum`).  training == 0 normalises with run_mean / run_var (required).  bn_save [4][C] = scale |
 * shift | mean | invstd is written in both BatchNorm modes.  ws: at least mlsp_thin_in_workspace_bytes(M, Cin, C) bytes.
 * Backward (same arguments as the forward saw; y is recomputed from X, H is not read): dW [C][Cin]; db [C] (nullable; exactly 0 in training
 * with BatchNorm); dgamma, dbeta [C] with BatchNorm.  There is no gradient for X. */
size_t mlsp_thin_in_workspace_bytes(int M, int Cin, int C);
int mlsp_thin_in_fwd_f32(const float* X, int ldx, int M, int Cin, const float* W, const float* bias, int C, const float* gamma, const float* beta,
                         float* run_mean, float* run_var, float momentum, float eps, int training, int act, float* H, float* bn_save, double* xmom,
                         void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_thin_in_bwd_f32(const float* dH, const float* X, int ldx, int M, int Cin, const float* W, const float* bias, int C, const float* gamma,
                         const float* beta, const float* bn_save, const double* xmom, int training, int act, float* dW, float* db, float* dgamma,
                         float* dbeta, void* ws, size_t ws_bytes, mlsp_stream_t stream);

/* Token pooling (Models.py:498 cat([x[:,0], x[:,1:].max(1)[0]])): y [B L][d] -> out [B][2 d] = y[b L] | max over the rows 1 .. L-1 of cloud b,
 * arg [B][d] = the row of that maximum, local to the cloud.  Strict comparison: the lowest row wins ties.  arg is always in [1, L): a NaN
 * never displaces a number, and an all-NaN column takes row 1 and reports NaN.  L >= 2, d % 4 == 0, 16-byte-aligned pointers.
 * Backward: dy [B L][d] is written completely (row 0 = the first half of dOut, row arg = the second half, 0 elsewhere). */
int mlsp_token_pool_fwd_f32(const float* y, int B, int L, int d, float* out, int32_t* arg, mlsp_stream_t stream);
int mlsp_token_pool_bwd_f32(const float* dOut, const int32_t* arg, int B, int L, int d, float* dy, mlsp_stream_t stream);

/* The two stages of the Point Transformer models (hengshuang_model.py) that no other entry covers (pyramid.hip).  fp32 rows of C channels;
 * no atomics, every sum in a fixed order: results are bit-identical run to run.  Limits: C % 4 == 0 and 16-byte-aligned feat / add / out /
 * dout / dfeat / X / dOut / dX (so 16-byte-aligned rows) -- anything else returns MLSP_ERR_UNSUPPORTED, launches nothing and leaves the
 * outputs untouched.  No entry reaches a matrix core.
 *
 * Upsample-and-add (TransitionUp): out [B][N][C] = add [B][N][C] + sum_{j<3} w_j feat[b][idx[b][n][j]], feat [B][S][C], idx / dist [B][N][3]
 * as mlsp_knn_query_f32 leaves them (entries in [0, S)), w_j = (1 / (dist_j + 1e-8)) / sum_j' (1 / (dist_j' + 1e-8)) -- the weights and the
 * summation order of mlsp_interp3_fwd_f32.  S == 1: out = add + feat[b][0], idx / dist may be NULL; S == 2 is MLSP_ERR_UNSUPPORTED.
 * Backward: dfeat [B][S][C] over the reverse index of idx (mlsp_group_reverse(idx, B, N, S, 3, ...)), one writer per element, list order;
 * S == 1: the sum of the cloud's rows of dout, accumulated in double, and dist / rev_off / rev_ent may be NULL.  The gradient of `add` is
 * dout itself. */
int mlsp_interp3_add_fwd_f32(const float* feat, const int32_t* idx, const float* dist, const float* add, int B, int N, int S, int C, float* out,
                             mlsp_stream_t stream);
int mlsp_interp3_add_bwd_f32(const float* dout, const float* dist, const int32_t* rev_off, const int32_t* rev_ent, int B, int N, int S, int C,
                             float* dfeat, mlsp_stream_t stream);

/* Cloud mean (points.mean(1)): X [B N][C] -> out [B][C] = the mean over the N rows of cloud b.  Every thread adds its rows in double from
 * the first addition, the partial sums are added in ascending order in double, and the quotient is rounded to fp32 once: the result is
 * within half an fp32 ulp plus N 2^-53 sum |x| / N of the exact mean.  Backward: dX [B N][C] = dOut[b] / N, written completely. */
int mlsp_cloud_mean_fwd_f32(const float* X, int B, int N, int C, float* out, mlsp_stream_t stream);
int mlsp_cloud_mean_bwd_f32(const float* dOut, int B, int N, int C, float* dX, mlsp_stream_t stream);

/* Training-batch preparation in one launch, one workgroup per cloud (PointDA/data/dataloader.py __getitem__: scale_to_unit_cube,
 * rotate_shape, farthest_point_sample_np, random_rotate_one_axis, jitter_pointcloud).  raw [B][Nmax] rows of >= 3 floats (pitch ld);
 * cloud b has counts[b] <= Nmax points (counts NULL: Nmax each).  Stages of cloud b, in this order:
 *   unit cube     c = mean, r = max |x - c| in double, u = f32((x - c) / r)          unless flags[b] & 8 (the coordinates pass through)
 *   pre-rotation  v = f32((u0 R[0][k] + u1 R[1][k]) + u2 R[2][k]) in double, R = Rpre + 9 b (row-major)           if flags[b] & 1
 *   sampling      farthest point sampling of S points on v in fp32 from start[b] (clamped into the cloud), first index wins ties;
 *                 S == counts[b]: nothing is sampled, idx = 0 .. S-1
 *   post-rotation the same product with Rpost + 9 b                                                                 if flags[b] & 2
 *   jitter        f32(f64(w) + min(max(sigma noise[b][i][k], -clip), clip))                                         if flags[b] & 4
 * -> out [B][S][3], idx [B][S] (int32, local to the cloud).  counts and flags are HOST arrays, read during the call (flags NULL: 0);
 * start [B], Rpre / Rpost [B][9], noise [B][S][3] are device arrays and may be NULL when no cloud's count / flags ask for them.
 * counts[b] <= 8192 (MLSP_ERR_UNSUPPORTED beyond); S <= counts[b], non-null required operands (MLSP_ERR_ARG otherwise) -- checked for
 * every cloud before anything is launched.  A cloud of identical points has r = 0: its output is NaN, its idx [start, 0, 0, ...]. */
int mlsp_batch_prepare_f32(const float* raw, int ld, int B, int Nmax, const int* counts, int S, const int* flags, const int* start,
                           const double* Rpre, const double* Rpost, const double* noise, double sigma, double clip, float* out, int* idx,
                           mlsp_stream_t stream);

/* Segmentation supervision (PointSegDA/trainer.py:221-233, 253-258: nn.CrossEntropyLoss on logits.permute(0, 2, 1), logits.max(dim=2)[1],
 * seg_metrics) from one read of the logits (segsup.hip).  logits fp32 [B][N][C], contiguous in C, row pitch ld >= C (cloud pitch N ld);
 * labels int64 [B][N].  Limits: 1 <= C <= 64, B >= 1, N >= 1, B N < 2^31 -- anything else returns MLSP_ERR_UNSUPPORTED and launches
 * nothing.  Rows are read as 16-byte quads where C % 4 == 0, ld % 4 == 0 and logits is 16-byte aligned, element by element otherwise.
 * No entry reaches a matrix core or takes a product mode.  Integer counters are added with LDS atomics; every floating-point sum is
 * taken in double in a fixed order (points of a thread, threads of a chunk, chunks of a cloud, clouds of the batch, each ascending): the
 * results are bit-identical run to run.
 *
 * A label outside [0, C) -- torch's ignore_index -100 among them -- is never used as an index: its point adds nothing to the loss, to the
 * valid-point count or to the metric counters, and its gradient row is 0; its lse and pred are still written.  (torch raises for such a
 * label other than ignore_index.)
 *
 * Forward, two launches: lse [B][N] double = m + log sum_c exp(x_c - m) (exps in fp32, sum and log in double); loss_pt [B][N] fp32
 * (nullable) = lse - x[label], 0 at ignored points; pred [B][N] int64 = the index of the maximum, the LOWEST index on ties (a NaN logit
 * gives a NaN loss and a pred somewhere in [0, C)); stats [B + 1][5] double: row b = loss sum | mIoU | accuracy | valid points | mean
 * loss of cloud b, row B = mean loss over the batch's valid points | their number | 0 | 0 | 0; mean [1] fp32 (nullable) = the mean loss rounded once.
 * mIoU: the mean over the classes with true[c] + pred[c] > 0 of tp[c] / (true[c] + pred[c] - tp[c]) in double from integer counts, the
 * quotients taken in ascending c and added in the order of numpy's add.reduce (eight running sums from eight classes on) --
 * sklearn.metrics.jaccard_score(average='macro') bit for bit; accuracy = correct / valid.  A cloud without a valid
 * point has NaN metrics; a batch without one a NaN mean.  ws: at least mlsp_seg_workspace_bytes(B, N, C) bytes (0: shape refused).
 * Backward, one launch: dlogits [B][N][C] (contiguous, written completely) = (exp(x - lse) - [c == label]) g with g = g_pt[b][n]
 * (reduction 'none') or g_mean[0] / stats[B][1] (reduction 'mean'); exactly one of g_pt and g_mean is non-NULL.
 * Metrics alone: labels and preds int64 [B][N] -> stats as above with the loss fields 0, through the same counters and finaliser.  A pred
 * outside [0, C) at a valid point counts for its label's class and as a miss, and for no predicted class. */
size_t mlsp_seg_workspace_bytes(int B, int N, int C);
int mlsp_seg_ce_fwd_f32(const float* logits, int ld, const int64_t* labels, int B, int N, int C, double* lse, float* loss_pt, int64_t* pred,
                        double* stats, float* mean, void* ws, size_t ws_bytes, mlsp_stream_t stream);
int mlsp_seg_ce_bwd_f32(const float* logits, int ld, const int64_t* labels, const double* lse, int B, int N, int C, const float* g_pt,
                        const float* g_mean, const double* stats, float* dlogits, mlsp_stream_t stream);
int mlsp_seg_metrics_i64(const int64_t* labels, const int64_t* preds, int B, int N, int C, double* stats, void* ws, size_t ws_bytes,
                         mlsp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MLSP_HIP_H */
