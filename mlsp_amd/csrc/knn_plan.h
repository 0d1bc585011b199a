// Which kernel one kNN search runs on, decided in ONE place (host only: no HIP header, no kernel; tools/knn_plan_host_check sweeps it on a
// CPU).  knn_plan() is pure arithmetic over the shape, the pitch, two alignments and the plane workspace at hand; launch_knn (knn.hip)
// builds a plan and follows it, mlsp_knn_f32 (api.hip) sizes the planes from the plan of the same call with every byte on offer, and the
// knn6*_supported predicates of launchers.h are statements over it.  The family table, in ladder order, is DESIGN.md section 27.
#pragma once
#include <stddef.h>
#include "../../include/mlsp_hip.h"

#define KNN_QB 64      // VALU kernel: queries per workgroup
#define KNN_TJ 32      // VALU kernel: candidates per LDS tile per wave
#define KM_STRIDE 33   // v3 / v4 / v5: row stride (floats) of a channel row of an operand tile
#define KNN4_CAP 64    // v4: survivors per query buffer
#define KNN5_CAP 32    // v5, KB = 0: keys per query and half
#define KNN5_CAPT 88   // v5, KB = 1: keys per query, both halves together (16-byte aligned rows)
#define K6_KMAX 24     // largest k of knn6_kernel
#define K6W_KMAX 40    // ... of knn6w_kernel
#define K6_LSTR 232    // v6: bytes between lists (58 dwords: 16 consecutive lists start in 16 different even banks)
#define KNN_LDS_MAX ((size_t)160 * 1024)

// ---- dynamic LDS of each family, as its kernel carves it
static inline size_t knn_lds_bytes(int KMAX, int C, bool runtime_c) {
    size_t tiles = (size_t)4 * KNN_TJ * C + 4 * KNN_TJ + (runtime_c ? (size_t)KNN_QB * (C + 1) : 0);
    size_t merge = (size_t)3 * KMAX * 64 * 2;
    return (tiles > merge ? tiles : merge) * sizeof(float);
}
static inline size_t knn3_lds_bytes(int CT) { return ((size_t)2 * CT * KM_STRIDE + 96) * sizeof(float); }
static inline size_t knn4_lds_bytes(int CT) { return ((size_t)2 * CT * KM_STRIDE + 96 + 2 * 4 * 32 * KNN4_CAP) * sizeof(float); }
static inline size_t knn5_lds_bytes(int CT, int N, bool res, bool kb, bool vec = false) {
    size_t tile = (size_t)CT * KM_STRIDE;
    if ((CT == 64 || (CT == 128 && !kb)) && !res && vec && (size_t)32 * (CT + 8) > tile) tile = (size_t)32 * (CT + 8);     // pass-A images (kernel: TILE_ALLOC)
    const size_t keys = kb ? (size_t)2 * 128 * KNN5_CAPT : (size_t)2 * 4 * 2 * 32 * KNN5_CAP;     // floats
    const size_t fl = (res ? (size_t)(N / 32) * tile + N : 4 * tile + 192) + keys + 128 + 256;
    return fl * sizeof(float);
}
static inline size_t knn6_lds_bytes(int N) { return (size_t)512 * K6_LSTR + (size_t)N * 4 + 128 * 4 + 512 * 4 + 64 + (size_t)8 * 512 * 4 + 512 * 4; }

// ---- the plane workspace of the v6 families
static inline int knn6_padded_channels(int C) { return C <= 16 ? 16 : C <= 64 ? 64 : 128; }
// image (bf16 hi | lo) + centred norms + the wide kernel's cloud flags (B <= P / 128 ints)
static inline size_t knn6_plane_bytes(int P, int C) { return (size_t)P * 2 * knn6_padded_channels(C) * 2 + (size_t)P * sizeof(float) + ((size_t)P / 128 + 4) * sizeof(int); }
static inline size_t knn6_vex_bytes(int P) { return (size_t)P * 16; }      // the cloud's {x, xx} image

// The question.  planes_avail: bytes of plane workspace at hand (0: none); planes16: it starts on a 16-byte boundary.
struct KnnAsk {
    int B = 0, N = 0, C = 0, k = 0, ld = 0;
    bool x16 = true;                                        // x starts on a 16-byte boundary
    size_t planes_avail = 0; bool planes16 = true;
};

enum KnnFamily { KNN_FAM_VEX, KNN_FAM_V6, KNN_FAM_V6W_V5, KNN_FAM_V5, KNN_FAM_V4, KNN_FAM_V3, KNN_FAM_VALU };

// knn_mfma5_kernel<CT, VEC, RES, KB> and its launch (512 threads); ok: v5 takes the shape
struct Knn5Plan { bool ok = false; int CT = 0; bool vec = false, res = false, kb = false; size_t lds = 0; unsigned grid_x = 0; };

// The answer.  status != MLSP_OK: what launch_knn returns, nothing launched.  CT: the kernel's channel tile (VALU: 3 = compile-time
// channels, 0 = run-time C); KMAX: VALU only.  v5: the family's own kernel (V5) or the one behind the wide kernel (V6W_V5) -- lds / grid /
// block are then the wide kernel's.  norm_pass: sqnorm_kernel runs first (the v6 families' prep kernels write the norms themselves).
struct KnnPlan {
    int status = MLSP_OK;
    KnnFamily family = KNN_FAM_VALU;
    int CT = 0, KMAX = 0;
    Knn5Plan v5;
    bool vec = false;                                       // v3 / v4: 16-byte row loads (the kernels' vec_ok argument)
    bool norm_pass = false;
    size_t lds = 0; unsigned grid_x = 0, grid_y = 1, block = 0;
    size_t plane_bytes = 0;                                 // what the family takes from the plane workspace
};

// v5: N % 128 == 0 (full query chunks, an even number of 32-candidate tiles), k <= 64, C <= 128, and an instantiation that fits
static inline Knn5Plan knn5_plan(const KnnAsk& q) {
    Knn5Plan v;
    const int N = q.N, C = q.C, k = q.k;
    if (N % 128 != 0 || k > 64 || C > 128) return v;
    v.kb = k > 24;        // k = 25..32 on the 64-maxima bound overflow its 32-key buffers too often (734 us vs 290 at N = 2048)
    v.CT = C <= 4 ? 4 : C <= 16 ? 16 : C <= 64 ? 64 : 128;
    v.vec = (C == v.CT) && (q.ld % 4 == 0) && q.x16;
    v.res = v.CT <= 16 && knn5_lds_bytes(v.CT, N, true, v.kb) <= KNN_LDS_MAX;
    v.lds = knn5_lds_bytes(v.CT, N, v.res, v.kb, v.vec);
    v.grid_x = (unsigned)(N / 128) * q.B;
    // k > 24 with 64 < C < 128 or unaligned rows: out of registers, stays on the list-merge kernel
    v.ok = v.lds <= KNN_LDS_MAX && !(v.CT == 128 && !v.vec && v.kb);
    return v;
}

// whole 128-query chunks of a cloud the v6 skeleton holds (N <= nmax), C <= cmax channels
static inline bool knn6_shape(const KnnAsk& q, int nmax, int cmax) {
    return q.B > 0 && q.N >= 128 && q.N % 128 == 0 && q.N <= nmax && q.C >= 1 && q.C <= cmax && q.k >= 1 && q.k <= q.N && knn6_lds_bytes(q.N) <= KNN_LDS_MAX;
}

static inline KnnPlan knn_plan(const KnnAsk& q) {
    KnnPlan p;
    const int B = q.B, N = q.N, C = q.C, k = q.k;
    if (B <= 0 || N <= 0 || C <= 0 || k <= 0 || k > N || q.ld < C) { p.status = MLSP_ERR_ARG; return p; }
    const int P = B * N;
    const bool vec = q.ld % 4 == 0 && q.x16;
    auto planes = [&q](size_t need) { return q.planes16 && q.planes_avail >= need; };
    auto v6 = [&](KnnFamily f, int CT, unsigned chunk, size_t need) {       // the v6 skeleton: 512 threads per `chunk` queries
        p.family = f; p.CT = CT; p.lds = knn6_lds_bytes(N); p.grid_x = (unsigned)(N / chunk) * B; p.block = 512; p.plane_bytes = need;
        return p;
    };
    auto tiles = [&](KnnFamily f, int CT, size_t lds, bool flat) {          // v3 / v4: 256 threads per 128 queries
        p.family = f; p.CT = CT; p.vec = vec; p.norm_pass = true; p.lds = lds; p.block = 256;
        p.grid_x = (unsigned)((N + 127) / 128) * (flat ? B : 1); p.grid_y = flat ? 1 : B;
        return p;
    };
    // C <= 3 (raw and transformed cloud), k <= 24, N <= 1024: the v6 skeleton with vector-exact sweeps (knn6.hip VEX)
    if (knn6_shape(q, 1024, 3) && k <= K6_KMAX && planes(knn6_vex_bytes(P))) return v6(KNN_FAM_VEX, 16, 128, knn6_vex_bytes(P));
    // v6: k <= 24 on whole 128-query chunks -- the five graph stages of DGCNN (C <= 16 stays on v5 until v6's selection phases beat it there)
    if (knn6_shape(q, 4096, 128) && k <= K6_KMAX && C > 16 && planes(knn6_plane_bytes(P, C)))
        return v6(KNN_FAM_V6, knn6_padded_channels(C), 128, knn6_plane_bytes(P, C));
    const Knn5Plan v5 = knn5_plan(q);
    // 24 < k <= 40 (PointSegDA's k = 40): the wide v6 kernel, with the v5 kernel behind it for the clouds it flags (list overflow: massive
    // ties; non-finite bounds) -- v5's workgroups of unflagged clouds return at once.  Only where v5 itself takes the shape.
    // Every C <= 128: at C = 3 (B = 16, N = 2048, k = 40) 82 us against v5's 117, C = 64 152 / 235, C = 128 210 / 435.
    if (knn6_shape(q, 4096, 128) && k > K6_KMAX && k <= K6W_KMAX && v5.ok && planes(knn6_plane_bytes(P, C))) {
        p.v5 = v5;
        return v6(KNN_FAM_V6W_V5, knn6_padded_channels(C), 64, knn6_plane_bytes(P, C));
    }
    // matrix-core kernels for every C <= 256 (the widest graph stage of the reference is 128 channels); beyond that only what the
    // VALU kernel's LDS tiles hold (C <= ~200 at k <= 40): MLSP_ERR_UNSUPPORTED otherwise
    if (C <= 256) {
        // two-pass threshold select pays once there are enough candidates per query (small clouds keep v3); 24 < k <= 64: 128 chunk maxima
        // per query need N >= 128
        const bool two_pass = k <= 32 && C <= 128 && N >= 256;
        if (v5.ok && (two_pass || (k > 24 && k <= 64 && C <= 128 && N >= 128))) {
            p.family = KNN_FAM_V5; p.v5 = v5; p.CT = v5.CT; p.norm_pass = true; p.lds = v5.lds; p.grid_x = v5.grid_x; p.block = 512;
            return p;
        }
        if (two_pass) { const int CT = C <= 4 ? 4 : C <= 16 ? 16 : C <= 64 ? 64 : 128; return tiles(KNN_FAM_V4, CT, knn4_lds_bytes(CT), true); }
        if (k <= 32) {                                          // lane-distributed lists
            const int CT = C <= 4 ? 4 : C <= 16 ? 16 : C <= 64 ? 64 : C <= 128 ? 128 : 256;
            return tiles(KNN_FAM_V3, CT, knn3_lds_bytes(CT), false);
        }
        // 32 < k <= 40 on a shape the two-pass kernel does not take (ragged N, N < 128, 64 < C < 128 or C > 128): the VALU kernel
    }
    p.family = KNN_FAM_VALU; p.CT = C == 3 ? 3 : 0; p.KMAX = k <= 20 ? 20 : 40; p.norm_pass = true;
    p.lds = knn_lds_bytes(p.KMAX, C, C != 3); p.grid_x = (unsigned)((N + KNN_QB - 1) / KNN_QB); p.grid_y = B; p.block = 256;
    if (k > 40 || p.lds > KNN_LDS_MAX) p.status = MLSP_ERR_UNSUPPORTED;
    return p;
}

// ---- the predicates of launchers.h: the shape reaches that family once the planes are there (C <= 16 at k <= 24 included: knn6_kernel takes
// it, the plan keeps it on v5); q: the shape's ask with contiguous, aligned rows and every byte of planes on offer
static inline KnnAsk knn_q(int B, int N, int C, int k) { KnnAsk q; q.B = B; q.N = N; q.C = C; q.k = k; q.ld = C; q.planes_avail = (size_t)-1; return q; }
static inline bool knn_q_vex_supported(int B, int N, int C, int k) { return knn6_shape(knn_q(B, N, C, k), 1024, 3) && k <= K6_KMAX; }
static inline bool knn_q_v6_supported(int B, int N, int C, int k) { return knn6_shape(knn_q(B, N, C, k), 4096, 128) && k <= K6_KMAX; }
static inline bool knn_q_v6w_supported(int B, int N, int C, int k) { return knn6_shape(knn_q(B, N, C, k), 4096, 128) && k > K6_KMAX && k <= K6W_KMAX; }
