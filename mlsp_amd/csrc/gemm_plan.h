// What one GEMM launch will do, decided in ONE place (host only: no HIP header, no kernel; tools/gemm_plan_host_check sweeps it on a CPU).
// gemm_plan() is pure arithmetic over the product mode, the shape and WHICH options the launch carries; launch_gemm (gemm.hip) builds a
// plan and follows it, and the shape queries of launchers.h (gemm_stat_parts, gemm_xf_supported, ...) are statements over the plan of the
// same shape -- with the slab present and no `accumulate` -- so a query and the launcher cannot disagree about ns / kts / bm or the kernel.
#pragma once
#include <stddef.h>
#include "../../include/mlsp_hip.h"

#define BM 128
#define BN 128
#define BK 32
#define SX_XF_KMAX 1024          // channels (K range of one workgroup) of an A-side operand transform in gemm_split_kernel

// How many K splits a launch will use (shared by the launcher and mlsp_workspace_bytes).
static inline int gemm_pick_split(int M, int N, int K) {
    int ntm = (M + BM - 1) / BM, ntn = (N + BN - 1) / BN;
    long tiles = (long)ntm * ntn;
    int ktiles = (K + BK - 1) / BK;
    if (tiles >= 256 || ktiles < 4) return 1;
    long want = (512 + tiles - 1) / tiles;          // aim at ~2 blocks per CU (measured: 320 is 35 % slower on the wgrad shapes; 768 / 1024 and 64-row tiles for the split launches: no gain)
    int ns = (int)(want < ktiles / 2 ? want : ktiles / 2);
    if (ns < 1) ns = 1;
    if (ns > 256) ns = 256;
    return ns;
}
// mode 2: does a contraction of `ktiles` K-tiles per workgroup go to the split kernel?  Short K loops stay on the fp32 kernel (measured per
// launch on the headline step, tools/cmp_dump.py, and per shape, tools/x6/lib_bench: the split kernel's longer prologue loses at K = 64 and,
// at K = 128, on grids too small to hide it: few rows AND a single column tile)
static inline bool gemm_split_pays(int M, int N, int ktiles) {
    return ktiles >= 8 || (ktiles >= 4 && (N >= 256 || M >= 16384));
}
// 64-row tiles when the 128-row grid is too small to keep ~3 workgroups per CU busy (and K is not split)
static inline int gemm_pick_bm(int mode, int M, int N, int K) {
    long tiles128 = (long)((M + 127) / 128) * ((N + BN - 1) / BN);
    // the split kernel amortises its operand split over the tile: 128 rows unless the grid would not fill the 512 workgroup slots
    const long few = (mode == 2 && gemm_split_pays(M, N, (K + BK - 1) / BK)) ? 512 : 1536;
    return (gemm_pick_split(M, N, K) == 1 && tiles128 < few && M >= 256) ? 64 : 128;
}
// A 64 x 64 weight gradient over many rows (dW = dY^T X of a 64 -> 64 layer over the edges of a set-abstraction level): neither the 128-row
// tile kernels (a quarter of the tile used, predicated path) nor the N = 64 kernel (M % 128) fit it.  With contiguous operands two
// consecutive rows are ONE row of a [K/2][128] matrix, and  A2^T B2  (128 x 128, an interior-tile launch) holds the even-row sum in its
// upper-left 64 x 64 block and the odd-row sum in its lower-right one: dW = their sum.  Twice the products on the fast kernel instead of four
// times on the slow one (configs[3]: 216 -> 70 us per step).
static inline bool gemm_fold64(bool ta, bool tb, int M, int N, int K, int lda, int ldb) {
    return ta && !tb && M == 64 && N == 64 && lda == 64 && ldb == 64 && K % 64 == 0 && K >= 8192;
}

// The question: product mode, shape, and which options the launch carries (GemmOpts, common.h).  A `*_ok` flag says that the fields of
// that option passed the launcher's pointer / pitch validation; a query asks with all of them true.
struct GemmAsk {
    int mode = 0; bool split_half = false;                  // CallCtx::mode() / split_half()
    bool ta = false, tb = false; int M = 0, N = 0, K = 0, lda = 0, ldb = 0, ldc = 0;
    bool a16 = true, b16 = true;                            // A / B start on a 16-byte boundary
    bool bias = false, bias_a4 = true, gbias = false; int rows_per_group = 0;
    bool stat = false, sel = false, sel_ok = true, accumulate = false;
    int xf = 0; bool xf_drop = false, xf_ok = true;         // transform side (GemmXf::which, 0: none), its dropout, its fields
    bool thin_xf = false;                                   // thin.hip transforms this shape (thin_xf_supported): its kernels are offered the launch first
    bool grp = false; int gmode = 0, G = 0; bool grp_ok = true;   // GemmGroups (grp_ok: the groups' B operands of mode 1)
    bool bs = false, bs_ok = true, dy = false, dy_ok = true;
    size_t slab_floats = 0;                                 // split-K slab at hand (0: none)
};

enum GemmFamily { GEMM_FAM_FOLD64, GEMM_FAM_N64, GEMM_FAM_F32_EDGE /* bounds-checked */, GEMM_FAM_F32 /* interior tiles */, GEMM_FAM_BF16, GEMM_FAM_SPLIT };

// The answer.  status != MLSP_OK: what launch_gemm returns without launching, AFTER the offers that were already made when the check
// failed (offer_*: thin.hip / skinny.hip take the launch if it is their shape -- their own tests, pointer alignment among them -- before
// the status or the family below count).  family FOLD64: the launcher folds and runs the plan of the 128 x 128 x K/2 product instead.
struct GemmPlan {
    int status = MLSP_OK;
    bool offer_thin = false, offer_skinny = false;
    GemmFamily family = GEMM_FAM_F32_EDGE;
    int ns = 1, kts = 0, bm = 128, ntm = 0, ntn = 0;        // K splits, K tiles per split, tile rows, row / column tiles
    size_t slab_need = 0;                                   // slab floats that splitting K takes (0: one pass whatever the slab)
    bool pays = false;                                      // mode 2 and a K range per workgroup long enough for the split kernel
    int ldc = 0;                                            // pitch of what the kernel writes (the slab's under split-K)
    bool a_vec = false, b_vec = false, fast = false, fast_out = false, xf_split = false;
    int xcd_map = 0, gtiles = 1;
    unsigned grid_x = 0, grid_y = 1;
    bool pieces = false;                                    // eligible for the two-piece f16 products (given a workspace tail and operand bounds)
};

// ns / kts / bm / tiles / the panel-major grid of a launch: the part of the plan that launch_gemm_mx shares
static inline void gemm_plan_tiles(GemmPlan& p, int mode, int M, int N, int K, size_t slab_floats, bool accumulate) {
    int ns = gemm_pick_split(M, N, K);
    p.slab_need = ns > 1 ? (size_t)ns * M * N : 0;
    if (slab_floats < p.slab_need) ns = 1;                      // no slab: fall back to one pass
    if (accumulate) ns = 1;                                     // beta = 1 lives in the one-pass epilogue
    const int ktiles = (K + BK - 1) / BK;
    p.kts = (ktiles + ns - 1) / ns;
    p.ns = (ktiles + p.kts - 1) / p.kts;
    p.bm = (p.ns == 1) ? gemm_pick_bm(mode, M, N, K) : 128;
    p.ntm = (M + p.bm - 1) / p.bm; p.ntn = (N + BN - 1) / BN;
    p.pays = mode == 2 && gemm_split_pays(M, N, p.kts);
    p.xcd_map = p.ntm >= 16 && p.ntn > 1;
    p.grid_x = (unsigned)(p.xcd_map ? ((p.ntm + 7) / 8) * 8 * p.ntn : p.ntm * p.ntn); p.grid_y = (unsigned)p.ns;
}

// interior tiles and 16-byte loads of a (d', y) pair launch (GemmDy) at the split count a slab allows
static inline bool gemm_dy_shape(const GemmAsk& q) {
    if (q.mode != 2 || q.tb) return false;
    if (q.M <= 32 || q.N < 32 || q.K <= 32) return false;
    GemmPlan t; gemm_plan_tiles(t, q.mode, q.M, q.N, q.K, (size_t)-1, false);
    const bool vec = q.lda % 4 == 0 && q.a16 && q.ldb % 4 == 0 && q.b16;
    if (!t.pays || (!q.ta && t.kts * BK > SX_XF_KMAX)) return false;
    return vec && q.M % t.bm == 0 && q.N % BN == 0 && q.K % BK == 0 && (long)(q.ta ? q.K : q.M) * q.lda * 4 < (1L << 30) && (long)q.K * q.ldb * 4 < (1L << 30);
}
// do the MFMA tile kernels stage `xf` through the operand transform: interior tiles, 16-byte loads, at the split count a slab allows
// (on the split kernel the A-side transform keeps the scale / shift of a workgroup's K range in LDS: <= SX_XF_KMAX)
static inline bool gemm_xf_shape(const GemmAsk& q) {
    const bool ta = q.ta, tb = q.tb;
    if (q.xf == 1 ? ta : !(ta && !tb)) return false;
    if (q.M <= 32 || q.N < 32 || q.K < 32 || (ta && !tb && q.K <= 32)) return false;
    GemmPlan t; gemm_plan_tiles(t, q.mode, q.M, q.N, q.K, (size_t)-1, false);
    const bool vec = q.lda % 4 == 0 && q.a16 && q.ldb % 4 == 0 && q.b16;
    if (q.xf == 1 && t.pays && t.kts * BK > SX_XF_KMAX) return false;
    return vec && q.M % t.bm == 0 && q.N % BN == 0 && q.K % BK == 0 && (long)(ta ? q.M : q.K) * q.lda * 4 < (1L << 30) && (long)q.K * q.ldb * 4 < (1L << 30);
}
// gemm_xf_supported: some kernel behind launch_gemm transforms this operand (not in mode 1: the bf16 kernel has no transform)
static inline bool gemm_xf_gate(const GemmAsk& q) { return q.mode != 1 && (q.thin_xf || gemm_xf_shape(q)); }

static inline GemmPlan gemm_plan(const GemmAsk& q) {
    GemmPlan p;
    const bool ta = q.ta, tb = q.tb; const int M = q.M, N = q.N, K = q.K;
    const bool grp = q.grp;
    auto fail = [&p](int rc) { p.status = rc; return p; };
    if (M <= 0 || N <= 0 || K <= 0) return fail(MLSP_ERR_ARG);
    // a block-diagonal launch: interior-tile fp32 / split kernels only (the caller launches group by group otherwise)
    if (grp && (q.G < 2 || q.G > 4 || q.sel || q.gbias || q.mode == 1 || (ta && tb))) return fail(MLSP_ERR_UNSUPPORTED);
    if (q.xf && !q.xf_ok) return fail(MLSP_ERR_UNSUPPORTED);
    if (q.dy && (!q.dy_ok || q.gbias || q.sel || q.stat || (q.xf && q.xf != 2) || !gemm_dy_shape(q))) return fail(MLSP_ERR_UNSUPPORTED);
    const bool plain = !q.dy && !grp && !q.gbias && !q.stat && !q.sel && !q.accumulate;
    // one tiny dimension (3 coordinates, 3 / 16 outputs): streaming VALU kernels priced against HBM, not MFMA tiles (thin.hip)
    p.offer_thin = plain && (!q.xf || q.mode != 1);
    if (q.xf && !gemm_xf_gate(q)) return fail(MLSP_ERR_UNSUPPORTED);    // the caller materialises the operand
    if (plain && !q.xf && !q.bs && !q.bias && gemm_fold64(ta, tb, M, N, K, q.lda, q.ldb) && q.a16 && q.b16) {
        GemmPlan in; gemm_plan_tiles(in, q.mode, 128, 128, K / 2, (size_t)-1, false);
        if (q.slab_floats >= in.slab_need + 128 * 128) { p.family = GEMM_FAM_FOLD64; return p; }
    }
    // per-cloud layers (<= 32 rows, or a 32-deep wgrad): one-pass skinny kernels, no split-K slab (skinny.hip)
    p.offer_skinny = plain && !q.xf && !q.bs && ((!ta && M <= 32) || (ta && !tb && K <= 32));
    const int ns0 = gemm_pick_split(M, N, K);
    if (q.sel && (!q.sel_ok || ns0 != 1)) return fail(MLSP_ERR_ARG);
    if (q.gbias && q.rows_per_group <= 0) return fail(MLSP_ERR_ARG);
    if (q.stat && ns0 != 1) return fail(MLSP_ERR_ARG);                    // the caller must check gemm_stat_parts()
    // the BatchNorm-backward sums of the previous layer from a dgrad's output pass (GemmBs): split kernel, 128-row interior tiles, one K pass
    if (q.bs && (ta || tb || q.xf || q.bias || q.gbias || q.accumulate || q.stat || q.sel || !q.bs_ok || q.mode != 2 || M % 128 || N % BN || K % BK ||
                 q.lda % 4 || q.ldb % 4 || q.ldc % 4 || ns0 != 1 || gemm_pick_bm(q.mode, M, N, K) != 128 || !gemm_split_pays(M, N, K / BK)))
        return fail(MLSP_ERR_UNSUPPORTED);
    gemm_plan_tiles(p, q.mode, M, N, K, q.slab_floats, q.accumulate);
    const int ns = p.ns, kts = p.kts, bm = p.bm, ksplit = kts * BK;
    p.a_vec = q.lda % 4 == 0 && q.a16; p.b_vec = q.ldb % 4 == 0 && q.b16;
    p.ldc = ns > 1 ? N : q.ldc;
    // FAST: every tile interior (M, N, K-range multiples of the tile), 16-byte loads legal on both operands
    // (byte offsets inside an operand tile's K range are 32-bit buffer offsets)
    const long a_span = ta ? (long)ksplit * q.lda * 4 : 128L * q.lda * 4 + (long)ksplit * 4;
    const long b_span = !tb ? (long)ksplit * q.ldb * 4 : 128L * q.ldb * 4 + (long)ksplit * 4;
    p.fast = p.a_vec && p.b_vec && M % bm == 0 && N % BN == 0 && K % BK == 0 && a_span < (1L << 31) - 4096 && b_span < (1L << 31) - 4096;
    // lean output pass: every row of a tile takes the same per-cloud bias row, byte offsets inside a wave's region fit 31 bits
    p.fast_out = p.fast && (!q.gbias || q.rows_per_group % bm == 0) && (long)p.ldc * 4 * 64 < (1L << 30);
    if (grp) {
        const int dim = q.gmode == 1 ? N : M, per = dim / q.G, tile = q.gmode == 1 ? BN : bm;   // columns (mode 1) / rows (mode 2) of one group
        if (!(p.fast && (q.gmode == 1 || q.gmode == 2) && per * q.G == dim && per % tile == 0 && (q.gmode != 1 || q.grp_ok))) return fail(MLSP_ERR_UNSUPPORTED);
        p.gtiles = per / tile;
    }
    // THE predicate "this launch runs on gemm_split_kernel" (a transform: where the split kernel takes it, the fp32 transform kernels otherwise)
    p.xf_split = q.xf && p.fast && p.pays && (q.xf != 1 || ksplit <= SX_XF_KMAX);
    const bool split_like = p.fast && p.pays && (!q.xf || p.xf_split);
    if (grp && q.xf && !p.xf_split) return fail(MLSP_ERR_UNSUPPORTED);   // (the fp32 transform kernels take no groups)
    // split-K launches of the split kernel with few row panels (weight gradients): XCD-grouped (split, panel) order, see the kernel
    if (!p.xcd_map && ns > 1 && split_like) {
        if (ns % 8 == 0 && p.ntm > 1) p.xcd_map = 3;                     // (all tiles of a split on one XCD)
        else if (p.ntn > 1 && (p.ntm * ns) % 8 == 0) p.xcd_map = 2;
        if (p.xcd_map) { p.grid_x = (unsigned)(p.ntm * p.ntn * ns); p.grid_y = 1; }
    }
    // (mode 1, N = 64: the bf16 kernel's tiles are 128 columns wide, so these launches used to fall to the bounds-checked f32 kernel at half-empty
    // tiles -- 33 us where the 64-column f32 kernel takes 12; exact products are within what mode 1 promises.)
    const bool n64 = !q.dy && !grp && !q.xf && N == 64 && p.a_vec && p.b_vec && M % 128 == 0 && K % BK == 0 && !(ta && tb) && !q.gbias &&
                     (!q.stat || (bm == 128 && ns == 1)) && !q.sel && (!q.bias || (ns == 1 && q.bias_a4)) && (ns == 1 || p.ldc == N);
    const bool on_split = split_like && !n64;
    p.pieces = q.split_half && on_split;
    if (n64) { p.family = GEMM_FAM_N64; p.grid_x = (unsigned)(M / 128); p.grid_y = (unsigned)ns; return p; }
    // the instantiations that exist (gemm.hip gemm_pick_kernel names them)
    bool have = true;
    if (q.dy) have = on_split && (!grp || q.gmode == (ta ? 2 : 1)) && (ta || !q.xf);
    else if (p.xf_split) have = q.xf == 1 ? (!ta && tb && (!grp || q.gmode == 1)) : (ta && !tb && (!grp || q.gmode == 2));
    else if (grp) have = q.gmode == 1 ? !ta : (ta && !tb);
    if (!have) return fail(MLSP_ERR_UNSUPPORTED);
    p.family = on_split ? GEMM_FAM_SPLIT : (q.xf || grp) ? GEMM_FAM_F32 : !p.fast ? GEMM_FAM_F32_EDGE : q.mode == 1 ? GEMM_FAM_BF16 : GEMM_FAM_F32;
    return p;
}

// Which kernel sums the slabs of a split-K launch (gemm.hip launch_splitk_reduce_any follows it).  aligned16: slab, C, bias and gbias all
// start on 16-byte boundaries; unfold: the caller offered an aligned unfold_dw (GemmOpts), the launch has no bias / gbias and M is even.
// VEC<ZG>: 16 bytes per lane over a contiguous C, ZG slab groups per workgroup; WAVE: one wave per output element (few outputs, many
// slabs); SCALAR: everything else (N % 4, a pitched C, a pointer 4 bytes off); UNFOLD<ZG>: VEC<ZG>'s sums written in the EdgeConv layout.
enum GemmReduce { GEMM_RED_VEC8, GEMM_RED_VEC4, GEMM_RED_VEC1, GEMM_RED_WAVE, GEMM_RED_SCALAR, GEMM_RED_UNFOLD8, GEMM_RED_UNFOLD4, GEMM_RED_UNFOLD1 };
static inline GemmReduce gemm_pick_reduce(int M, int N, int ldc, int ns, bool aligned16, bool unfold) {
    const size_t total = (size_t)M * N;
    const bool vec = N % 4 == 0 && ldc == N && aligned16;
    if (vec) {      // enough workgroups to fill the chip: more slab groups per workgroup when the output is small
        const int zg = (ns >= 32 && total / 4 <= 64 * 1024) ? 8 : ns >= 8 ? 4 : 1;
        if (unfold) return zg == 8 ? GEMM_RED_UNFOLD8 : zg == 4 ? GEMM_RED_UNFOLD4 : GEMM_RED_UNFOLD1;
        return zg == 8 ? GEMM_RED_VEC8 : zg == 4 ? GEMM_RED_VEC4 : GEMM_RED_VEC1;
    }
    return (ns >= 32 && total <= 256 * 1024) ? GEMM_RED_WAVE : GEMM_RED_SCALAR;
}
// Mode 3, a launch eligible for the two-piece f16 products (GemmPlan::pieces) whose operand bounds are not all at hand: does MEASURING
// `mbytes` bytes of operands pay?  The three-product kernel saves about a third of the six-product launch (~150 TF on these shapes); a
// measuring pass streams the operand at ~3 TB/s plus a launch.  Nothing to measure: it pays.
static inline bool gemm_pieces_measure_pays(int M, int N, int K, double mbytes) {
    const double gain_us = 0.33 * (2.0 * M * N * K) / 150e6, cost_us = 3.0 + mbytes / 3e6;
    return !(mbytes > 0.0 && gain_us < cost_us);
}

// ---- the shape queries of launchers.h as statements over the plan of a launch of that shape with its slab and no `accumulate`
// (gemm.hip binds them to a CallCtx and to the operands' alignment; q: that shape's ask with no option set and slab_floats = (size_t)-1)
static inline GemmPlan gemm_q_tiles(int mode, int M, int N, int K) { GemmPlan t; gemm_plan_tiles(t, mode, M, N, K, (size_t)-1, false); return t; }
static inline int gemm_q_stat_parts(int mode, int M, int N, int K) { const GemmPlan t = gemm_q_tiles(mode, M, N, K); return t.ns == 1 ? t.ntm : 0; }
static inline int gemm_q_panel_rows(int mode, int M, int N, int K) { return gemm_q_tiles(mode, M, N, K).bm; }
static inline size_t gemm_q_slab_floats(int M, int N, int K) {      // (the same in every mode; thin.hip's own slab comes on top, gemm.hip)
    size_t a = gemm_q_tiles(0, M, N, K).slab_need;
    if (gemm_fold64(true, false, M, N, K, 64, 64)) {                // the folded launch's slab + its 128 x 128 result
        const size_t f = gemm_q_slab_floats(128, 128, K / 2) + 128 * 128;
        a = a > f ? a : f;
    }
    return a;
}
static inline bool gemm_q_xf_supported(GemmAsk q, int which, bool thin_xf) { q.xf = which; q.thin_xf = thin_xf; return gemm_xf_gate(q); }
static inline bool gemm_q_xf_on_split(int mode, int M, int N, int K, int which) {
    const GemmPlan t = gemm_q_tiles(mode, M, N, K);
    return t.pays && (which != 1 || t.kts * BK <= SX_XF_KMAX);
}
static inline int gemm_q_bs_parts(GemmAsk q) { q.bs = true; return gemm_plan(q).status == MLSP_OK ? q.M / 128 : 0; }
static inline bool gemm_q_dy_supported(GemmAsk q) {
    q.dy = true;
    const GemmPlan p = gemm_plan(q);
    return p.status == MLSP_OK && p.family == GEMM_FAM_SPLIT;
}
