// Host check of the GEMM dispatch plan (mlsp_amd/csrc/gemm_plan.h): the one function that decides what a launch of a given shape does,
// and the shape queries that are statements over it.  Five parts:
//   agreement  over a grid of shapes x layouts x pitches x product modes, a query that says yes implies a launchable plan with that option
//              set; where the logic inherited from before the plan disagrees with itself, the shapes are listed below, by value;
//   pins       the plan of every GEMM launch of one BASELINE configs[1] step and one configs[4] step, as the library listed them on an
//              MI355X (MLSP_PROF_DUMP, tools/r6/gemm_dump.py and tools/time_config4.py) before the plan existed;
//   corners    the folded 64 x 64 weight gradient and the N = 64 kernel, by hand;
//   reach      one "reach p<prec>:<label> <- ta tb M N K bias" line (the smallest such product) per distinct label that plain and bias launches of a grid of shapes meet, as mlsp_gemm_f32 makes
//              them (contiguous operands, the slab at hand, no operand bound at hand), up to the largest product the tests launch;
//   plans      one "plan" line per line of stdin
//                  `prec ta tb M N K lda ldb ldc a16 b16 bias bias_a4 bias_a16 slab_floats`   (slab_floats -1: whatever the launch asks)
//              (tests/test_gemm_plan_cpu.py pins the kernel each test shape reaches with them).
// Labels: FAMILY/bm/ns=<n>/xcd=<m>[/fast][/pieces | /pieces:six][/thin?][/skinny?] -- pieces: mode 3 and eligible for the two-piece f16
// products; ":six": measuring both operands does not pay (gemm_pieces_measure_pays), so the launch stays on the six bf16 products;
// thin? / skinny?: thin.hip / skinny.hip are offered the launch first.  FOLD64:<label of the 128 x 128 x K/2 launch it runs>.  A plan line
// of a split-K launch names the kernel that sums its slabs.
// A stand-alone program that needs no GPU and no HIP header:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gemm_plan_host_check/main.cpp
//       -o build/gemm_plan_host_check && build/gemm_plan_host_check < /dev/null
#include "../../mlsp_amd/csrc/gemm_plan.h"
#include <initializer_list>
#include <map>
#include <stdio.h>
#include <string>


static int fails = 0;
#define EXPECT(c) do { if (!(c)) { if (++fails < 25) printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static GemmAsk bare(int prec, bool ta, bool tb, int M, int N, int K, int pad) {
    GemmAsk q;
    q.mode = prec == 3 ? 2 : prec; q.split_half = prec == 3;        // what CallCtx makes of the ABI's `precision`
    q.ta = ta; q.tb = tb; q.M = M; q.N = N; q.K = K;
    q.lda = (ta ? M : K) + pad; q.ldb = (tb ? K : N) + pad; q.ldc = N + pad;
    q.slab_floats = (size_t)-1;
    return q;
}

// ---- agreement ------------------------------------------------------------------------------------------------------------------
static const int Ms[] = {1, 32, 33, 64, 128, 192, 256, 320, 4096, 16384, 32768, 65536, 262144};
static const int Ns[] = {3, 16, 32, 64, 128, 192, 256, 512, 1024};
static const int Ks[] = {3, 32, 64, 96, 128, 256, 512, 1024, 2048, 32768};

// The one place where the logic inherited from before the plan disagrees with itself, by value: gemm_xf_supported says yes to an A-side
// transform (which = 1) of a product in the dgrad layout (A row-major, B k-major) wherever the tiles are interior, but where that launch
// would run on the split kernel -- these (M, N, K) at pitches dim and dim + 4, precision 2 and 3 -- no instantiation transforms A in that
// layout and launch_gemm answers MLSP_ERR_UNSUPPORTED.  No caller asks (api.hip and multi.hip transform A in the forward layout only,
// DESIGN.md); the plan reproduces it, this pull request does not change it.
static const int XF_A_DGRAD_ON_SPLIT[][3] = {
    {4096, 256, 1024}, {4096, 256, 2048}, {4096, 512, 512}, {4096, 512, 1024}, {4096, 512, 2048}, {4096, 1024, 128},
    {4096, 1024, 256}, {4096, 1024, 512}, {4096, 1024, 1024}, {16384, 128, 512}, {16384, 128, 1024}, {16384, 128, 2048},
    {16384, 256, 128}, {16384, 256, 256}, {16384, 256, 512}, {16384, 256, 1024}, {16384, 512, 128}, {16384, 512, 256},
    {16384, 512, 512}, {16384, 512, 1024}, {16384, 1024, 128}, {16384, 1024, 256}, {16384, 1024, 512}, {16384, 1024, 1024},
    {32768, 128, 128}, {32768, 128, 256}, {32768, 128, 512}, {32768, 128, 1024}, {32768, 256, 128}, {32768, 256, 256},
    {32768, 256, 512}, {32768, 256, 1024}, {32768, 512, 128}, {32768, 512, 256}, {32768, 512, 512}, {32768, 512, 1024},
    {32768, 1024, 128}, {32768, 1024, 256}, {32768, 1024, 512}, {32768, 1024, 1024}, {65536, 128, 128}, {65536, 128, 256},
    {65536, 128, 512}, {65536, 128, 1024}, {65536, 256, 128}, {65536, 256, 256}, {65536, 256, 512}, {65536, 256, 1024},
    {65536, 512, 128}, {65536, 512, 256}, {65536, 512, 512}, {65536, 512, 1024}, {65536, 1024, 128}, {65536, 1024, 256},
    {65536, 1024, 512}, {65536, 1024, 1024}, {262144, 128, 128}, {262144, 128, 256}, {262144, 128, 512}, {262144, 128, 1024},
    {262144, 256, 128}, {262144, 256, 256}, {262144, 256, 512}, {262144, 256, 1024}, {262144, 512, 128}, {262144, 512, 256},
    {262144, 512, 512}, {262144, 512, 1024}, {262144, 1024, 128}, {262144, 1024, 256}, {262144, 1024, 512}, {262144, 1024, 1024},
};
static bool listed(int M, int N, int K) {
    for (const auto& s : XF_A_DGRAD_ON_SPLIT) if (s[0] == M && s[1] == N && s[2] == K) return true;
    return false;
}

static void agreement() {
    long points = 0, xf_yes = 0, dy_yes = 0, bs_yes = 0, stat_yes = 0, disagree = 0;
    for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int t = 0; t < 4; ++t) for (int pad : {0, 4, 1}) for (int prec = 0; prec < 4; ++prec) {
        const bool ta = t & 1, tb = t & 2;
        const GemmAsk q = bare(prec, ta, tb, M, N, K, pad);
        ++points;
        for (int which = 1; which <= 2; ++which) {
            if (!gemm_q_xf_supported(q, which, false)) continue;
            ++xf_yes;
            GemmAsk a = q; a.xf = which;
            const GemmPlan p = gemm_plan(a);
            const bool on_split = gemm_q_xf_on_split(q.mode, M, N, K, which);
            if (p.status != MLSP_OK) {      // only the listed shapes, and every one of them
                ++disagree;
                EXPECT(p.status == MLSP_ERR_UNSUPPORTED && which == 1 && !ta && !tb && on_split && q.mode == 2 && pad != 1 && listed(M, N, K));
                continue;
            }
            EXPECT((p.family == GEMM_FAM_SPLIT) == on_split);
            EXPECT(p.family == GEMM_FAM_SPLIT || p.family == GEMM_FAM_F32);
        }
        if (gemm_q_dy_supported(q)) {
            ++dy_yes;
            GemmAsk a = q; a.dy = true;
            const GemmPlan p = gemm_plan(a);
            EXPECT(p.status == MLSP_OK && p.family == GEMM_FAM_SPLIT && p.fast && !tb);
            if (!ta) EXPECT(p.kts * BK <= SX_XF_KMAX);
        }
        if (!ta && !tb) {
            const int parts = gemm_q_bs_parts(q);
            if (parts > 0) {
                ++bs_yes;
                GemmAsk a = q; a.bs = true;
                const GemmPlan p = gemm_plan(a);
                EXPECT(p.status == MLSP_OK && p.ns == 1 && p.bm == 128 && parts == M / 128 && p.ntm == parts && p.family == GEMM_FAM_SPLIT);
            }
        }
        {
            const int parts = gemm_q_stat_parts(q.mode, M, N, K);
            GemmAsk a = q; a.stat = true;
            const GemmPlan p = gemm_plan(a);
            if (parts > 0) { ++stat_yes; EXPECT(p.status == MLSP_OK && p.ns == 1 && parts == p.ntm && p.bm == gemm_q_panel_rows(q.mode, M, N, K)); }
            else EXPECT(p.status == MLSP_ERR_ARG);
        }
        {
            const GemmPlan p = gemm_plan(q);
            EXPECT(p.status == MLSP_OK);
            if (p.family != GEMM_FAM_FOLD64) EXPECT(p.ns == 1 || gemm_q_slab_floats(M, N, K) >= (size_t)p.ns * M * N);
            GemmAsk a = q; a.slab_floats = 0;                   // without a slab, or under beta = 1, a launch is one pass
            EXPECT(gemm_plan(a).ns == 1);
            a = q; a.accumulate = true;
            EXPECT(gemm_plan(a).ns == 1);
        }
    }
    printf("agreement: %ld points; yes: xf %ld, dy %ld, bs %ld, stat %ld; listed disagreements: %ld\n", points, xf_yes, dy_yes, bs_yes, stat_yes, disagree);
    EXPECT(points == 13L * 9 * 10 * 4 * 3 * 4);
    EXPECT(xf_yes > 1000 && dy_yes > 100 && bs_yes > 10 && stat_yes > 1000);
    EXPECT(disagree == 4L * (long)(sizeof XF_A_DGRAD_ON_SPLIT / sizeof XF_A_DGRAD_ON_SPLIT[0]));      // 2 pitches x 2 precisions of each
}

// ---- corners -------------------------------------------------------------------------------------------------------------------------
static void corners() {
    for (int prec = 0; prec < 4; ++prec) {
        // the folded weight gradient: (64, 64, 8192) A^T B with both pitches 64 and room for the inner launch's slab + its 128 x 128 result
        GemmAsk q = bare(prec, true, false, 64, 64, 8192, 0);
        q.slab_floats = gemm_q_slab_floats(64, 64, 8192);
        EXPECT(q.slab_floats == (size_t)64 * 128 * 128 + 128 * 128);          // 64 splits (half its 128 K tiles) of the 128 x 128 x 4096 product
        GemmPlan p = gemm_plan(q);
        EXPECT(p.status == MLSP_OK && p.family == GEMM_FAM_FOLD64 && p.offer_thin && !p.offer_skinny);
        q.slab_floats -= 1;                                                   // a float short: the ordinary tiles (a quarter of a 128 x 128 tile used)
        p = gemm_plan(q);
        EXPECT(p.status == MLSP_OK && p.family == GEMM_FAM_F32_EDGE && p.ntm == 1 && p.ntn == 1 && p.bm == 128 && !p.fast);
        EXPECT(p.ns == 128 && p.kts == 2 && p.grid_x == 1 && p.grid_y == 128 && !p.pieces);
        q = bare(prec, true, false, 64, 64, 8192, 4);                         // pitch 68: two rows are not one row of a [K/2][128] matrix
        EXPECT(gemm_plan(q).family == GEMM_FAM_F32_EDGE);
        q = bare(prec, true, false, 64, 64, 8192, 0); q.bias = true;
        EXPECT(gemm_plan(q).family == GEMM_FAM_F32_EDGE);
        q = bare(prec, true, false, 64, 64, 4096, 0);                         // K < 8192: not worth folding
        EXPECT(gemm_plan(q).family == GEMM_FAM_F32_EDGE);
        q = bare(prec, true, false, 64, 64, 8192, 0); q.a16 = false;
        EXPECT(gemm_plan(q).family == GEMM_FAM_F32_EDGE);

        // N = 64: the 64-column kernel takes whole 128-row panels only, in every layout but A^T B^T
        q = bare(prec, false, true, 256, 64, 128, 0);
        p = gemm_plan(q);
        EXPECT(p.status == MLSP_OK && p.family == GEMM_FAM_N64 && p.ns == 2 && p.kts == 2 && p.grid_x == 2 && p.grid_y == 2 && !p.pieces);
        q.slab_floats = 0;
        p = gemm_plan(q);
        EXPECT(p.family == GEMM_FAM_N64 && p.ns == 1 && p.grid_x == 2 && p.grid_y == 1);
        q = bare(prec, false, true, 192, 64, 128, 0);                         // M % 128 != 0
        p = gemm_plan(q);
        EXPECT(p.status == MLSP_OK && p.family == GEMM_FAM_F32_EDGE && p.ns == 2 && p.bm == 128 && p.ntm == 2 && p.ntn == 1 && p.grid_x == 2 && p.grid_y == 2);
        q = bare(prec, false, true, 320, 64, 128, 0);
        EXPECT(gemm_plan(q).family == GEMM_FAM_F32_EDGE);
        q = bare(prec, true, true, 256, 64, 128, 0);
        EXPECT(gemm_plan(q).family == GEMM_FAM_F32_EDGE);
        q = bare(prec, false, true, 256, 64, 128, 0); q.bias = true;          // a bias under split-K is added by the slab reduce, which this kernel's callers skip
        EXPECT(gemm_plan(q).family == GEMM_FAM_F32_EDGE);
        q.slab_floats = 0;
        EXPECT(gemm_plan(q).family == GEMM_FAM_N64);
        q = bare(prec, false, true, 262144, 64, 64, 0); q.stat = true;        // statistics: where the panels are 128 rows (2048 tiles >= 1536), one pass
        p = gemm_plan(q);
        EXPECT(p.family == GEMM_FAM_N64 && p.bm == 128 && p.ns == 1 && p.grid_x == 2048 && p.ntm == 2048);
        q = bare(prec, false, true, 256, 64, 64, 0); q.stat = true;           // 64-row panels chosen: the tile kernels keep the statistics layout
        p = gemm_plan(q);
        EXPECT(p.status == MLSP_OK && p.bm == 64 && p.family != GEMM_FAM_N64);
    }
    // statuses in the launcher's order: an argument error behind an offer still lets thin.hip try first
    GemmAsk q = bare(0, false, true, 4096, 16, 64, 0); q.bias = true;
    GemmPlan p = gemm_plan(q);
    EXPECT(p.status == MLSP_OK && p.offer_thin && !p.offer_skinny);
    q = bare(0, false, true, 16, 256, 64, 0);
    p = gemm_plan(q);
    EXPECT(p.offer_thin && p.offer_skinny);
    q.stat = true;
    p = gemm_plan(q);
    EXPECT(!p.offer_thin && !p.offer_skinny && p.status == MLSP_OK);
    q = bare(2, false, true, 4096, 256, 1024, 0); q.grp = true; q.G = 5; q.gmode = 1;     // 8 splits of 4 K tiles: pays at N >= 256
    EXPECT(gemm_plan(q).status == MLSP_ERR_UNSUPPORTED);
    q.G = 2;
    p = gemm_plan(q);
    EXPECT(p.status == MLSP_OK && p.family == GEMM_FAM_SPLIT && p.gtiles == 1);
    q.mode = 0;
    p = gemm_plan(q);
    EXPECT(p.status == MLSP_OK && p.family == GEMM_FAM_F32);
    q.M = 0;
    EXPECT(gemm_plan(q).status == MLSP_ERR_ARG);
}

// ---- pins ------------------------------------------------------------------------------------------------------------------------------
// One line per GEMM-family launch of one step, in launch order, as the library built from the commit before the plan listed them on an
// MI355X (MLSP_PROF_DUMP: layout, shape, split, bm, epilogue bits, split family) joined with that run's kernel trace (kernel, grid).
// configs[1]: tools/r6/gemm_dump.py, precision 3 (f16x3); configs[4]: C4_MODE=bf16 tools/time_config4.py, precision 1 with bf16 storage,
// whose launches with a bf16 operand or result (mx) go through launch_gemm_mx and take the tiling part of the plan only.
// stat / sel: the listing's epilogue bits; xf / dy: template arguments of the kernel that ran; pieces: eligible for the f16 pieces.
struct Pin { int prec, mx, ta, tb, M, N, K, stat, sel, xf, dy; GemmFamily family; int ns, bm; unsigned grid_x, grid_y; int pieces; };
static const Pin PINS[] = {
    // configs[1]
    {3, 0, 0, 1,  32768,  1024,    128, 1, 1, 0, 0, GEMM_FAM_SPLIT, 1, 128, 2048, 1, 1},
    {3, 0, 0, 1,  32768,   128,     64, 0, 0, 0, 0, GEMM_FAM_F32, 1, 64, 512, 1, 0},
    {3, 0, 0, 1,  32768,   256,     64, 0, 0, 0, 0, GEMM_FAM_F32, 1, 64, 1024, 1, 0},
    {3, 0, 0, 1,  32768,   512,    128, 0, 0, 0, 0, GEMM_FAM_SPLIT, 1, 128, 1024, 1, 1},
    {3, 0, 0, 1,  32768,  1024,    512, 1, 1, 0, 0, GEMM_FAM_SPLIT, 1, 128, 2048, 1, 1},
    {3, 0, 0, 1,  32768,  1024,    512, 1, 0, 0, 0, GEMM_FAM_SPLIT, 1, 128, 2048, 1, 1},
    {3, 0, 0, 1,  32768,   512,    256, 1, 0, 1, 0, GEMM_FAM_SPLIT, 1, 128, 1024, 1, 1},
    {3, 0, 0, 1,  32768,   256,    512, 1, 0, 1, 0, GEMM_FAM_SPLIT, 1, 128, 512, 1, 1},
    {3, 0, 0, 1,  32768,   256,    256, 1, 0, 1, 0, GEMM_FAM_SPLIT, 1, 128, 512, 1, 1},
    {3, 0, 0, 1,  32768,   256,    256, 1, 0, 1, 0, GEMM_FAM_SPLIT, 1, 128, 512, 1, 1},
    {3, 0, 0, 0,  32768,   512,    128, 0, 0, 0, 1, GEMM_FAM_SPLIT, 1, 128, 1024, 1, 1},
    {3, 0, 1, 0,    256,   256,  32768, 0, 0, 2, 1, GEMM_FAM_SPLIT, 128, 128, 512, 1, 1},
    {3, 0, 0, 0,  32768,   256,    256, 0, 0, 0, 1, GEMM_FAM_SPLIT, 1, 128, 512, 1, 1},
    {3, 0, 1, 0,    256,   256,  32768, 0, 0, 2, 1, GEMM_FAM_SPLIT, 128, 128, 512, 1, 1},
    {3, 0, 0, 0,  32768,   512,    256, 0, 0, 0, 1, GEMM_FAM_SPLIT, 1, 128, 1024, 1, 1},
    {3, 0, 1, 0,    512,   256,  32768, 0, 0, 2, 1, GEMM_FAM_SPLIT, 64, 128, 512, 1, 1},
    {3, 0, 0, 0,  32768,   512,    256, 0, 0, 0, 1, GEMM_FAM_SPLIT, 1, 128, 1024, 1, 1},
    {3, 0, 1, 0,    256,   512,  32768, 0, 0, 2, 1, GEMM_FAM_SPLIT, 64, 128, 512, 1, 1},
    {3, 0, 0, 0,  32768,   512,   1024, 0, 0, 0, 1, GEMM_FAM_SPLIT, 1, 128, 1024, 1, 1},
    {3, 0, 1, 0,   1024,   512,  32768, 0, 0, 0, 1, GEMM_FAM_SPLIT, 16, 128, 512, 1, 1},
    {3, 0, 1, 0,    512,   512,  32768, 0, 0, 0, 0, GEMM_FAM_SPLIT, 32, 128, 512, 1, 1},
    {3, 0, 0, 0,   1024,   512,    512, 0, 0, 0, 0, GEMM_FAM_F32, 8, 128, 32, 8, 0},
    {3, 0, 1, 0,    512,   512,   1024, 0, 0, 0, 0, GEMM_FAM_F32, 16, 128, 16, 16, 0},
    {3, 0, 0, 0,  32768,   512,    512, 0, 0, 0, 0, GEMM_FAM_SPLIT, 1, 128, 1024, 1, 1},
    {3, 0, 0, 0,  32768,   128,    512, 0, 0, 0, 0, GEMM_FAM_SPLIT, 1, 64, 512, 1, 1},
    {3, 0, 1, 0,    512,   128,  32768, 0, 0, 0, 0, GEMM_FAM_SPLIT, 128, 128, 512, 1, 1},
    {3, 0, 0, 0,  32768,    64,    256, 0, 0, 0, 0, GEMM_FAM_N64, 1, 64, 256, 1, 0},
    {3, 0, 1, 0,    256,    64,  32768, 0, 0, 0, 0, GEMM_FAM_N64, 256, 128, 2, 256, 0},
    {3, 0, 0, 0,  32768,    64,    128, 0, 0, 0, 0, GEMM_FAM_N64, 1, 64, 256, 1, 0},
    {3, 0, 1, 0,    128,    64,  32768, 0, 0, 0, 0, GEMM_FAM_N64, 256, 128, 1, 256, 0},
    {3, 0, 1, 0,    128,   128,  32768, 0, 0, 0, 0, GEMM_FAM_F32, 256, 128, 1, 256, 0},
    {3, 0, 0, 0,   1024,   128,    128, 0, 0, 0, 0, GEMM_FAM_F32, 2, 128, 8, 2, 0},
    {3, 0, 1, 0,    128,   128,   1024, 0, 0, 0, 0, GEMM_FAM_F32, 16, 128, 1, 16, 0},
    {3, 0, 0, 0,  32768,   128,    128, 0, 0, 0, 0, GEMM_FAM_SPLIT, 1, 64, 512, 1, 1},
    // configs[4]
    {1, 0, 0, 1,  32768,  1024,    128, 0, 1, 0, 0, GEMM_FAM_BF16, 1, 128, 2048, 1, 0},
    {1, 0, 0, 1,  32768,   128,     64, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 512, 1, 0},
    {1, 0, 0, 1,  32768,   128,     64, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 512, 1, 0},
    {1, 0, 0, 1,  32768,  1024,    192, 0, 1, 0, 0, GEMM_FAM_BF16, 1, 128, 2048, 1, 0},
    {1, 1, 0, 1,  32768,   256,    192, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   256,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   128,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 512, 1, 0},
    {1, 1, 0, 1,  32768,   256,    192, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   256,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   128,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 512, 1, 0},
    {1, 1, 0, 1,  32768,   256,    192, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   256,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   128,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 512, 1, 0},
    {1, 1, 0, 1,  32768,   512,    192, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 2048, 1, 0},
    {1, 1, 0, 1,  32768,   256,    512, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   256,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   256,    192, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   256,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 0, 1,  32768,   128,    256, 1, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 512, 1, 0},
    {1, 1, 0, 0,  32768,   256,    128, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    128,   256,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 256, 128, 2, 256, 0},
    {1, 1, 0, 0,  32768,   256,    256, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    256,   256,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 128, 128, 4, 128, 0},
    {1, 1, 0, 0,  32768,   192,    256, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    256,   192,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 128, 128, 4, 128, 0},
    {1, 1, 0, 0,  32768,   256,    256, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    256,   256,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 128, 128, 4, 128, 0},
    {1, 1, 0, 0,  32768,   512,    256, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 2048, 1, 0},
    {1, 1, 1, 0,    256,   512,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 64, 128, 8, 64, 0},
    {1, 1, 0, 0,  32768,   192,    512, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    512,   192,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 64, 128, 8, 64, 0},
    {1, 1, 0, 0,  32768,   256,    128, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    128,   256,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 256, 128, 2, 256, 0},
    {1, 1, 0, 0,  32768,   256,    256, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    256,   256,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 128, 128, 4, 128, 0},
    {1, 1, 0, 0,  32768,   192,    256, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    256,   192,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 128, 128, 4, 128, 0},
    {1, 1, 0, 0,  32768,   256,    128, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    128,   256,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 256, 128, 2, 256, 0},
    {1, 1, 0, 0,  32768,   256,    256, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    256,   256,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 128, 128, 4, 128, 0},
    {1, 1, 0, 0,  32768,   192,    256, 0, 0, 0, 0, GEMM_FAM_BF16, 1, 64, 1024, 1, 0},
    {1, 1, 1, 0,    256,   192,  32768, 0, 0, 0, 0, GEMM_FAM_BF16, 128, 128, 4, 128, 0},
    {1, 0, 0, 0,  32768,    64,    128, 0, 0, 0, 0, GEMM_FAM_N64, 1, 64, 256, 1, 0},
    {1, 0, 1, 0,    128,    64,  32768, 0, 0, 0, 0, GEMM_FAM_N64, 256, 128, 1, 256, 0},
    {1, 0, 0, 0,  32768,    64,    128, 0, 0, 0, 0, GEMM_FAM_N64, 1, 64, 256, 1, 0},
    {1, 0, 1, 0,    128,    64,  32768, 0, 0, 0, 0, GEMM_FAM_N64, 256, 128, 1, 256, 0},
};
static void pins() {
    int n = 0;
    for (const Pin& w : PINS) {
        ++n;
        GemmAsk q = bare(w.prec, w.ta, w.tb, w.M, w.N, w.K, 0);
        GemmPlan p;
        if (w.mx) { gemm_plan_tiles(p, q.mode, w.M, w.N, w.K, q.slab_floats, false); p.family = GEMM_FAM_BF16; }
        else { q.stat = w.stat; q.sel = w.sel; q.xf = w.xf; q.dy = w.dy; p = gemm_plan(q); }
        const bool same = p.status == MLSP_OK && p.family == w.family && p.ns == w.ns && p.bm == w.bm && p.grid_x == w.grid_x && p.grid_y == w.grid_y &&
                          p.pieces == (w.pieces != 0);
        if (!same) printf("pin %d: %c%c M=%d N=%d K=%d -> status %d family %d ns %d bm %d grid %u,%u pieces %d\n", n, w.ta ? 'T' : 'N', w.tb ? 'T' : 'N', w.M, w.N,
                          w.K, p.status, (int)p.family, p.ns, p.bm, p.grid_x, p.grid_y, (int)p.pieces);
        EXPECT(same);
    }
    EXPECT(n == 34 + 47);
}

// ---- labels, reach, plans ---------------------------------------------------------------------------------------------------------
static const char* const FAMILY_NAMES[] = {"FOLD64", "N64", "F32_EDGE", "F32", "BF16", "SPLIT"};
static const char* const REDUCE_NAMES[] = {"VEC8", "VEC4", "VEC1", "WAVE", "SCALAR", "UNFOLD8", "UNFOLD4", "UNFOLD1"};

// the 128 x 128 x K/2 launch a folded 64 x 64 weight gradient runs (gemm.hip launch_gemm): A^T B at pitch 128, its own slab, no bias
static GemmAsk fold_inner(const GemmAsk& q) {
    GemmAsk in = q;
    in.M = in.N = 128; in.K = q.K / 2; in.lda = in.ldb = in.ldc = 128; in.bias = false;
    in.slab_floats = gemm_q_slab_floats(128, 128, q.K / 2);
    return in;
}
static std::string label(const GemmAsk& q, const GemmPlan& p) {
    if (p.family == GEMM_FAM_FOLD64 && p.status == MLSP_OK) { const GemmAsk in = fold_inner(q); return "FOLD64:" + label(in, gemm_plan(in)); }
    std::string s;
    if (p.status != MLSP_OK) s = p.status == MLSP_ERR_ARG ? "ERR_ARG" : "ERR_UNSUPPORTED";
    else {
        s = std::string(FAMILY_NAMES[p.family]) + "/" + std::to_string(p.bm) + "/ns=" + std::to_string(p.ns) + "/xcd=" + std::to_string(p.xcd_map);
        if (p.fast) s += "/fast";
        // (mlsp_gemm_f32 finds no bound at hand: both operands as they lie in memory would be measured)
        if (p.pieces) s += gemm_pieces_measure_pays(q.M, q.N, q.K, 4.0 * ((double)q.M * q.K + (double)q.K * q.N)) ? "/pieces" : "/pieces:six";
    }
    if (p.offer_thin) s += "/thin?";
    if (p.offer_skinny) s += "/skinny?";
    return s;
}
// the slab sum of a launch through mlsp_gemm_f32 (slab and C on 16-byte boundaries, no unfold_dw); null: one pass
static const char* reducer(const GemmAsk& q, const GemmPlan& p, bool bias_a16) {
    if (p.status != MLSP_OK) return nullptr;
    if (p.family == GEMM_FAM_FOLD64) { const GemmAsk in = fold_inner(q); return reducer(in, gemm_plan(in), true); }
    return p.ns > 1 ? REDUCE_NAMES[gemm_pick_reduce(q.M, q.N, q.ldc, p.ns, !q.bias || bias_a16, false)] : nullptr;
}

// Shapes for the reach lines: every threshold of gemm_pick_split / gemm_pick_bm / gemm_split_pays / xcd_map / N64 / FOLD64 / the skinny
// offer from both sides, every count of 128-row panels below 16 (where xcd_map and the tile height turn) against wide N, up to
// M N K = 2^34 + 2^32 (the largest product the tests launch: 4096 x 2048 x 512 and 65536 x 1024 x 128 are 2^32 and 2^33).  Contiguous
// operands, as functional.gemm passes them unless told otherwise.
static void reach() {
    static const int Ms[] = {1, 32, 33, 64, 100, 128, 192, 256, 320, 384, 512, 640, 768, 896, 960, 1024, 1152, 1280, 1408, 1536, 1664, 1792, 1920, 2048, 4096, 16384, 32768, 65536};
    static const int Ns[] = {3, 16, 32, 64, 100, 128, 192, 256, 512, 1024, 1408, 1664, 2048, 2560, 4096, 4608, 4736, 8192, 16384};
    static const int Ks[] = {3, 32, 64, 96, 100, 128, 256, 512, 1024, 2048, 8192, 16384, 32768, 65536, 524288};
    std::map<std::string, std::string> seen;        // label -> the smallest product that meets it: "ta tb M N K bias"
    std::map<std::string, double> size;
    long points = 0;
    for (int prec = 0; prec < 4; ++prec) for (int M : Ms) for (int N : Ns) for (int K : Ks) for (int t = 0; t < 4; ++t) for (int bias = 0; bias < 2; ++bias) {
        if ((double)M * N * K > 17179869184.0 + 4294967296.0) continue;
        GemmAsk q = bare(prec, t & 1, t & 2, M, N, K, 0);
        q.bias = bias; q.slab_floats = gemm_q_slab_floats(M, N, K);
        const GemmPlan p = gemm_plan(q);
        ++points;
        EXPECT(p.status == MLSP_OK);
        const std::string l = "p" + std::to_string(prec) + ":" + label(q, p);
        const double mnk = (double)M * N * K;
        if (!seen.count(l) || mnk < size[l]) {
            size[l] = mnk;
            seen[l] = std::to_string(t & 1) + " " + std::to_string((t & 2) / 2) + " " + std::to_string(M) + " " + std::to_string(N) + " " + std::to_string(K) + " " + std::to_string(bias);
        }
    }
    for (const auto& s : seen) printf("reach %s <- %s\n", s.first.c_str(), s.second.c_str());
    printf("reach: %ld points, %zu labels\n", points, seen.size());
    EXPECT(seen.size() >= 40);
}

static void plans() {
    int prec, ta, tb, a16, b16, bias, bias_a4, bias_a16;
    long long slab;
    GemmAsk q;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %lld", &prec, &ta, &tb, &q.M, &q.N, &q.K, &q.lda, &q.ldb, &q.ldc, &a16, &b16, &bias, &bias_a4, &bias_a16,
                 &slab) == 15) {
        if (prec < 0 || prec > 3) { printf("plan: precision %d?\n", prec); ++fails; continue; }
        q.mode = prec == 3 ? 2 : prec; q.split_half = prec == 3;
        q.ta = ta; q.tb = tb; q.a16 = a16; q.b16 = b16; q.bias = bias; q.bias_a4 = bias_a4;
        q.slab_floats = slab < 0 ? gemm_q_slab_floats(q.M, q.N, q.K) : (size_t)slab;
        const GemmPlan p = gemm_plan(q);
        const char* red = reducer(q, p, bias_a16 != 0);
        printf("plan %d %d %d %d %d %d -> %s grid %u,%u vec %d%d reduce %s\n", prec, ta, tb, q.M, q.N, q.K, label(q, p).c_str(), p.grid_x, p.grid_y, (int)p.a_vec,
               (int)p.b_vec, red ? red : "-");
    }
}

int main() {
    agreement();
    pins();
    corners();
    reach();
    plans();
    if (fails) { printf("gemm_plan_host_check: %d FAILED\n", fails); return 1; }
    printf("gemm_plan_host_check: ok\n");
    return 0;
}
