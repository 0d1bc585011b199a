// kNN v6 (k <= 24, N % 128 == 0, N <= 4096, C <= 128): barrier-free approximate sweeps + exact resolution of the ambiguous survivors only.
// Replaces PointDA/model_utils.py:9-16 `knn` (twin PointSegDA/Models.py:8-15) for the wide graph stages of DGCNN (C = 64, 64, 128 at
// k = 20); same canonical arithmetic and total order as knn.hip / oracle/knn_canon.c, indices bit-exact.
//
// What v5 (knn.hip) spends its time on: one __syncthreads per 32-candidate tile (LDS staging shared by 8 waves), an exact f32-MFMA second
// sweep (64 matrix cycles per 2 channels), and a ballot / popcount / branch sequence per accumulator register in the survivor pass
// (~700 instructions per tile).  Here:
//   * knn6_prep_kernel splits every point ONCE into bf16 hi / lo pieces next to the canonical squared norms (it replaces sqnorm_kernel),
//     stored FRAGMENT-major: [32-point tile][16-channel block][hi | lo][half h][row][8 bf16] -- the 64 lanes of a wave fetch one MFMA
//     operand as ONE contiguous KiB (16 bytes per lane, every cache line used whole).  The sweeps load their fragments straight from
//     that image (L2-resident) into a register ring: no LDS staging, no conversion, NO barrier inside a sweep.
//   * TRANSPOSED tiles: A = 32 candidates, B = 32 queries, so a lane owns ONE query (column) and its 16 accumulator registers are 16
//     candidates of the tile.  Per-query state (threshold, survivor cursor) is per-lane: the survivor pass is v_cmpx / ds_write2 / add per
//     pair, no ballots, no scalar branches.  The accumulator starts at -xx_j / 2 (one LDS read per 4 rows), so a = dot' - xx_j / 2
//     orders like the distance and pd' = 2 a - xx_q.  A wave carries ONE query group (32 queries) against half the candidates, two waves
//     per SIMD (two groups per wave against the same fragments was measured and rejected: see the kernel's comment).
//   * BOTH sweeps use the split-bf16 products hi hi + lo hi + hi lo.  Error budget (worst case, not typical): bf16 has 8 significant
//     bits, so |x - hi| <= 2^-8 |x|, |x - hi - lo| <= 2^-16 |x|; the dropped terms (lo lo, the two residual products) are at most
//     3 x 2^-16 |x_q,c x_j,c| per channel, i.e. |2 dot' - 2 dot| <= 3 x 2^-16 (xx_q + xx_j) = 2^-14.4 (xx_q + xx_j); the fp32 accumulation
//     inside and between the 3 C / 16 MFMAs adds at most 2^-16.1 (xx_q + xx_j) at C = 128; the canonical value's own two roundings
//     2^-22.  Sum < 2^-13.9 (xx_q + xx_j): E = 2^-13 (xx_q + X), X >= xx_j, bounds it with a factor 1.9 to spare.
//     Pass A: 64 running maxima per query (16 registers x 2 half-wave lanes x 2 candidate halves), tau = their k-th largest: at least k
//     candidates have pd' >= tau, so the true k-th best is >= tau - E and every true neighbour has pd' >= tau - 2 E (X = the cloud's
//     largest squared norm): pass B keeps exactly those (~1.4 k of N).
//   * Coordinates: the sweeps run on x - x_first(cloud) (distances are translation invariant, the split products' error scales with the
//     norms of what is multiplied); the canonical value's own rounding on the RAW coordinates is budgeted separately:
//     E = 2^-13 (xc_q + Xc) + (C + 4) 2^-23 (xx_q + Xx), xc = centred, xx = raw squared norms.
//   * Exactness: a survivor whose pd' is farther than 2 E from its neighbours in rank (Xc = the largest centred norm among the query's
//     survivors) has its rank decided by pd' alone.  Four lanes per query sort the query's <= 32 survivors in registers (bitonic network, the
//     exchanges at distance 8 / 16 through v_permlane16 / 32_swap),
//     flags the gaps within 2 E, the flagged (~10-40 %) get their canonical distance from an fmaf chain over the fp32 rows (pairs packed
//     densely over the wave), and odd-even passes under the full order (value desc, index asc) settle the flagged runs -- safe, because
//     an unflagged value differs from its neighbours by more than 2 E and an exact one from its approximation by at most E.  Queries
//     with more than 32 survivors (or exact lists) take a counting path with the same logic.
//   * Any list overflow (massive ties: more than 24 survivors in a quarter of a query's candidates) or NaN / inf bound sends the whole
//     workgroup through an exact path: f32 MFMA tiles from the fp32 rows, per-lane sorted top-k lists in registers, the same final.
// Measured on MI355X (B = 32, N = 1024, k = 20, one call incl. the prep kernel; uniform random clouds): C = 64 71 us (v5 113), C = 128 103 us
// (v5 176), N = 2048 C = 64 95 us (v5 176); C = 3 54 us (v5 49: the selection phases dominate when the sweeps are trivial, so C <= 16 stays
// on v5).  Inside the DGCNN step (features of a 3-D manifold: small gaps between neighbours relative to the norms, 2-3x more ambiguous
// pairs): 89 / 129 us against 118 / 165.  Phase cycles per wave at C = 64, two waves per SIMD (clock stamps between the phases): sweeps 17 k + 27 k,
// tau 5.5 k, list conversion 5 k, sort / flag / settle 26 k, exact distances 16 k (bound by cache-line transactions: every 16-byte piece
// of a gathered row is its own transaction; a cooperative fetch through LDS lost to its chain of dependent steps as written here).
#include "common.h"
#include "knn_plan.h"      // K6_KMAX / K6W_KMAX / K6_LSTR, knn6_lds_bytes, the layout of the planes
#include <math.h>
#include <type_traits>

typedef __bf16 k6bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int k6u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int k6u32x4 __attribute__((ext_vector_type(4)));
typedef int k6i32x4 __attribute__((ext_vector_type(4)));

#define K6_CAP 24           // survivors one list (a query's candidates of one part and half-wave) keeps
#define K6_LENT 28          // entries of a list: the cursor is clamped every 4 appends
#define K6_EPS 1.220703125e-04f      // 2^-13 (error budget in the header)

// byte offset of the 16-byte piece (point row of its tile, half h) of block kb, plane p (0 hi, 1 lo) of tile T
__device__ __forceinline__ size_t k6_piece(size_t T, int nkb, int kb, int p, int h, int row) {
    return (((T * nkb + kb) * 2 + p) * 2 + h) * 512 + (size_t)row * 16;
}

// canonical squared norms xx (fmaf chain over the raw coordinates, c ascending: what the exact distances use) + the fragment-major bf16
// hi / lo image of every point RELATIVE TO THE FIRST POINT OF ITS CLOUD and the squared norms xc of those differences (P % 32 == 0).
// Distances do not change under a translation, the error of the split products scales with the NORMS of what is multiplied: features
// after BatchNorm + LeakyReLU + max sit far from the origin compared with their spread (squared norm ~14x the centred one at the first
// EdgeConv output), and bounds in terms of the raw norms would declare most survivors ambiguous.
template <int CT>
__global__ __launch_bounds__(256) void knn6_prep_kernel(const float* __restrict__ x, int ld, int P, int N, int C, float* __restrict__ xx,
                                                        float* __restrict__ xc, char* __restrict__ planes, int* __restrict__ idx, int k,
                                                        int* __restrict__ cloud_flag) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    if (cloud_flag && i < P / N) cloud_flag[i] = 0;           // (knn6w_kernel: which clouds go to the v5 kernel)
    // Every output row starts as k zeros: a query with fewer than k comparable candidates (NaN coordinates -- its own or its cloud's) keeps
    // index 0 in the positions the main kernel does not write, as oracle/knn_canon.c does; the gathers downstream never see an
    // uninitialised index.
    for (int s = 0; s < k; ++s) idx[(size_t)i * k + s] = 0;
    const float* r = x + (size_t)i * ld;
    const float* r0 = x + (size_t)(i / N) * N * ld;           // first point of the cloud
    const bool vec = (ld & 3) == 0 && (((uintptr_t)x) & 15) == 0;
    const size_t T = (size_t)(i >> 5);
    const int row = i & 31;
    float acc = 0.f, accc = 0.f;
#pragma unroll
    for (int c0 = 0; c0 < CT; c0 += 8) {
        float v[8], o[8];
        if (vec && c0 + 8 <= C) {
            const f32x4 a = *(const f32x4*)(r + c0), b = *(const f32x4*)(r + c0 + 4);
            const f32x4 a0 = *(const f32x4*)(r0 + c0), b0 = *(const f32x4*)(r0 + c0 + 4);
            v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
            o[0] = a0[0]; o[1] = a0[1]; o[2] = a0[2]; o[3] = a0[3]; o[4] = b0[0]; o[5] = b0[1]; o[6] = b0[2]; o[7] = b0[3];
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[e] = (c0 + e < C) ? r[c0 + e] : 0.f; o[e] = (c0 + e < C) ? r0[c0 + e] : 0.f; }
        }
        k6bf16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (c0 + e < C) acc = fmaf(v[e], v[e], acc);
            const float d = v[e] - o[e];
            accc = fmaf(d, d, accc);
            const __bf16 hv = (__bf16)d;
            hi[e] = hv;
            lo[e] = (__bf16)(d - (float)hv);
        }
        *(k6bf16x8*)(planes + k6_piece(T, CT / 16, c0 >> 4, 0, (c0 >> 3) & 1, row)) = hi;
        *(k6bf16x8*)(planes + k6_piece(T, CT / 16, c0 >> 4, 1, (c0 >> 3) & 1, row)) = lo;
    }
    xx[i] = acc;
    xc[i] = accc;
}

// VEX mode (C <= 3: the raw and the transformed cloud of DGCNN): no image, no centring -- the sweeps compute the CANONICAL distance itself
// with vector FMAs, so every survivor's value is exact and nothing has to be re-resolved.  Per point {x0, x1, x2, xx} (zero-padded
// coordinates: fmaf(0, 0, acc) == acc), xx = the canonical chain; the output rows start as zeros (see knn6_prep_kernel).
__global__ __launch_bounds__(256) void knn6_prep_vex_kernel(const float* __restrict__ x, int ld, int P, int C, float* __restrict__ xx,
                                                            f32x4* __restrict__ cand, int* __restrict__ idx, int k) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    for (int s = 0; s < k; ++s) idx[(size_t)i * k + s] = 0;
    const float* r = x + (size_t)i * ld;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    float acc = 0.f;
    for (int c = 0; c < C; ++c) { v[c] = r[c]; acc = fmaf(r[c], r[c], acc); }
    v[3] = acc;
    xx[i] = acc;
    cand[i] = v;
}

template <int I, int Nn, class F>
__device__ __forceinline__ void k6_static_for(F&& f) {
    if constexpr (I < Nn) { f(std::integral_constant<int, I>{}); k6_static_for<I + 1, Nn>(f); }
}

// candidate beats list entry (value desc, index asc); false for a NaN candidate
__device__ __forceinline__ bool k6_beats(float d, int j, float pv, int pi) { return d > pv || (d == pv && j < pi); }

// ------------------------------------------------------------------------------------------------------------------------------------
// The cut of a workgroup: 8 waves = QG groups of 32 queries x PARTS contiguous parts of the cloud's candidates; wave w carries group
// w % QG against part w / QG.  Everything else about the two kernels' geometry follows from QG:
//                                          knn6_kernel (k <= 24)     knn6w_kernel (24 < k <= 40)
//   QG     query groups                    4                         2
//   QWG    queries per workgroup           128                       64
//   PARTS  candidate parts per group       2 halves                  4 quarters
//   NL     lists per query (part x h)      4                         8
//   NMAX   pass-A maxima per query         64                        128
//   FL     lanes per query, fast final     4 (32 rank positions)     8 (64 rank positions)
//   KMAX   largest k                       K6_KMAX = 24              K6W_KMAX = 40
template <int QG_>
struct K6Cut {
    static constexpr int QG = QG_, QGS = __builtin_ctz(QG), QWG = 32 * QG, PARTS = 8 / QG, NL = 2 * PARTS, NMAX = 16 * NL;     // (QGS = log2 QG)
    static constexpr int KMAX = QG == 4 ? K6_KMAX : K6W_KMAX; // largest k the kernel is dispatched for
    static constexpr int XS = NMAX + 4;                       // floats per query of the tau exchange image (16-byte aligned rows, 4-bank skew)
    static constexpr int FL = NL, FQ = 64 / FL, FCAP = 8 * FL;       // fast final: lanes per query, queries per wave, survivors it holds
    // index of list t = 2 part + h of query qlc of group qg among the workgroup's 512 lists
    static __device__ __forceinline__ int list_at(int qg, int qlc, int t) { return (qg * NL + t) * 32 + qlc; }
};
typedef K6Cut<4> K6Narrow;
typedef K6Cut<2> K6Wide;

// prologue, norm bounds: nxx[j] = -xc_j / 2 (what the sweeps' accumulators start from) and this thread's share of the two maxima
// (fmaxf drops a NaN operand: a NaN norm -- a NaN coordinate, or an infinite first point of the cloud, the origin of the centred
// image -- becomes an infinite bound here, and an infinite bound sends the workgroup through the exact path / to the v5 kernel)
__device__ __forceinline__ void k6_fill_nxx(int tid, int N, const float* xcb, const float* xxb, float* nxx, float& m, float& mr) {
    for (int j = tid; j < N; j += 512) {
        const float v = xcb[j], w = xxb[j];
        nxx[j] = -0.5f * v; m = fmaxf(m, v == v ? v : INFINITY); mr = fmaxf(mr, w == w ? w : INFINITY);
    }
}
// ... and their reduction over the workgroup (one __syncthreads: nxx is complete behind it): xcmax = largest centred, xxmax = largest raw norm
__device__ __forceinline__ void k6_reduce_bounds(int lane, int wave, float m, float mr, float* red, float& xcmax, float& xxmax) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { m = fmaxf(m, __shfl_xor(m, o, 64)); mr = fmaxf(mr, __shfl_xor(mr, o, 64)); }
    if (lane == 0) { red[wave] = m; red[8 + wave] = mr; }
    __syncthreads();
    xcmax = red[0]; xxmax = red[8];
#pragma unroll
    for (int w = 1; w < 8; ++w) { xcmax = fmaxf(xcmax, red[w]); xxmax = fmaxf(xxmax, red[8 + w]); }
}

// MFMA operand of 16-channel block kb of the 32-point tile at `tile` (uniform address): row l31, channels 16 kb + 8 h .. + 7 of the hi and the
// lo plane; voff = h * 512 + l31 * 16, this lane's 16 bytes of a fragment: the wave reads one contiguous KiB per piece (k6_piece)
__device__ __forceinline__ void k6_frag_load(const char* tile, int kb, unsigned voff, k6bf16x8& fh, k6bf16x8& fl) {
    const char* p = tile + kb * 2048;
    fh = *(const k6bf16x8*)(p + voff);
    fl = *(const k6bf16x8*)(p + 1024 + voff);
}
// B operand: the wave's 32 queries = tile T of the image
template <int NKB>
__device__ __forceinline__ void k6_load_query(const char* planes, size_t T, unsigned voff, k6bf16x8 (&qh)[NKB], k6bf16x8 (&ql)[NKB]) {
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) k6_frag_load(planes + T * (NKB * 2048), kb, voff, qh[kb], ql[kb]);
}

// One sweep of a wave over its part of the candidates: nt 32-candidate tiles from cand0 (uniform: the part's first tile in the image),
// part * nt the part's first tile in the cloud.  sel(acc, tl) sees the finished 32 x 32 tile:
// acc[r] = a(query l31, candidate (r & 3) + 8 (r >> 2) + 4 h of the tile), a = dot' - xc_j / 2.
// Fragment ring: slot (tile % PF, block) is refilled right after its use with the tile PF ahead; a scheduling barrier after every
// refill keeps the loads where they are written (the scheduler otherwise sinks them next to their use: prefetch distance zero).
// The compiler drains the memory counter once per loop trip (its wait-count analysis merges pessimistically at the back edge), so a
// trip covers UNR tiles: the drain exposes one L2 latency per UNR tiles of MFMA work.
template <int NKB, class Sel>
__device__ __forceinline__ void k6_sweep(const char* cand0, unsigned voff, const float* nxx, int part, int h, int nt,
                                         const k6bf16x8 (&qh)[NKB], const k6bf16x8 (&ql)[NKB], Sel&& sel) {
    constexpr int PF = NKB >= 8 ? 1 : NKB >= 4 ? 2 : 4;      // tiles of fragments in flight (the ring holds PF * NKB blocks of 2 x 4 registers)
    constexpr int NR = PF * NKB;
    constexpr int UNR = NKB >= 8 ? 2 : 8;                     // tiles per loop trip (4 at C = 128 costs two spilled registers)
    auto frag_load = [&](int tl, int kb, k6bf16x8& ah, k6bf16x8& al) {       // A operand: candidate row l31 of tile tl of this part
        k6_frag_load(cand0 + (size_t)tl * (NKB * 2048), kb, voff, ah, al);
    };
    k6bf16x8 fh[NR], fl[NR];
    auto tile = [&](auto SLOT, auto RING, int tl, int tn) {   // tn: the tile that refills this ring slot (always loaded: no branch)
        constexpr int s0 = decltype(SLOT)::value * NKB;
        constexpr bool ring = decltype(RING)::value;
        f32x16 acc;
        const float* p = nxx + (part * nt + tl) * 32 + 4 * h;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 v = *(const f32x4*)(p + 8 * g4);
            acc[4 * g4] = v[0]; acc[4 * g4 + 1] = v[1]; acc[4 * g4 + 2] = v[2]; acc[4 * g4 + 3] = v[3];
        }
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh[s0 + kb], qh[kb], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl[s0 + kb], qh[kb], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh[s0 + kb], ql[kb], acc, 0, 0, 0);
            if (ring) {
                frag_load(tn, kb, fh[s0 + kb], fl[s0 + kb]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        sel(acc, tl);
    };
    const int nmain = (nt / UNR) * UNR;
    if (nmain > 0) {                                          // (so nt >= UNR >= PF: the ring's first PF tiles exist, no clamp)
#pragma unroll
        for (int tu = 0; tu < PF; ++tu)
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) frag_load(tu, kb, fh[tu * NKB + kb], fl[tu * NKB + kb]);
        for (int t0 = 0; t0 < nmain; t0 += UNR) {
            k6_static_for<0, UNR>([&](auto TU) {
                constexpr int tu = decltype(TU)::value;
                const int tl = t0 + tu;
                const int tn = min(tl + PF, nt - 1);          // (past the end the last tile is fetched again: harmless, and no branch in the body)
                tile(std::integral_constant<int, tu % PF>{}, std::true_type{}, tl, tn);
            });
        }
    }
    for (int tl = nmain; tl < nt; ++tl) {                     // ragged tail (nt not a multiple of UNR): one tile at a time through slot 0
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) frag_load(tl, kb, fh[kb], fl[kb]);
        tile(std::integral_constant<int, 0>{}, std::false_type{}, tl, tl);
    }
}

// pass A: a lane's 16 running maxima -> its 16 floats of the query's row of the tau exchange image (slot = 2 part + h)
__device__ __forceinline__ void k6_store_maxima(float* dst, const float (&cm)[16]) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) { const f32x4 v = {cm[4 * g4], cm[4 * g4 + 1], cm[4 * g4 + 2], cm[4 * g4 + 3]}; *(f32x4*)(dst + 4 * g4) = v; }
}

// 64 floats sorted descending in registers (bitonic network, one lane)
__device__ __forceinline__ void k6_sort64(float (&v)[64]) {
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < 64; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
                    if ((i & k2) == 0) { v[i] = hi; v[l] = lo; }           // descending overall
                    else { v[i] = lo; v[l] = hi; }
                }
            }
}

// pass B, one tile: the survivors (acc[r] >= thr) of the 16 candidates jb + (r & 3) + 8 (r >> 2) go to the list at LDS byte address `base`.
// per pair: v_cmpx (exec = survivors) / ds_write2_b32 {value, index} at the cursor / cursor += 8 under that mask / exec back to all lanes:
// three vector instructions and no branch; the cursor `ad` is clamped every 4 appends (lists have 4 entries of slack), `top` keeps the
// farthest it got (overflow: top > base + K6_CAP * 8).
#define K6_APPEND(ad_, val_, thr_, j_, gate_) asm volatile("v_cmpx_ge_f32_e32 vcc, %1, %2\n\tds_write2_b32 %0, %1, %3 offset1:1\n\tv_add_u32_e32 %0, 8, %0\n\ts_mov_b64 exec, -1" \
                                                           : "+v"(ad_) : "v"(val_), "v"(thr_), "v"(j_), "v"(gate_) : "vcc", "memory")
__device__ __forceinline__ void k6_append16(unsigned& ad, unsigned& top, unsigned base, const f32x16& acc, float thr, int jb) {
    int jv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) jv[r] = jb + (r & 3) + 8 * (r >> 2);
    // The compiler does not place the MFMA -> VALU / LDS read wait states for instructions INSIDE an asm statement: a visible VALU read of
    // the accumulator (gate) comes first -- the hazard recognizer pads in front of it -- and every append depends on the gate.
    const float gate = fmaxf(acc[0], acc[15]);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        K6_APPEND(ad, acc[r], thr, jv[r], gate);
        if ((r & 3) == 3) { top = max(top, ad); ad = min(ad, base + K6_CAP * 8); }
    }
}

// F0: a lane moves ITS list to the pd domain (pd' = 2 a - xc_q; `exact`: the list holds pd itself) and fills it to the end with {-inf, 0}
// (never ahead of, never close to a real entry: the counting loops of the slow final read whole blocks unmasked); the list's length and
// the largest centred norm among its survivors go to slot t = 2 part + h of query qs of the workgroup.
template <class Cut, bool VEX>
__device__ __forceinline__ void k6_f0(char* LB, int cnt, bool exact, float xcq, const float* nxx, int* cnts, float* lmn, int qs, int t) {
    float mn = 0.f;                                            // min of -xc_j / 2 = -(largest centred squared norm among this list's survivors) / 2
#pragma unroll
    for (int p0 = 0; p0 < K6_LENT; p0 += 4) {
        k6u32x2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = *(const k6u32x2*)(LB + (p0 + u) * 8);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float a = __int_as_float((int)v[u][0]);
            const float p = (exact || VEX) ? a : fmaf(2.0f, a, -xcq);
            const bool live = p0 + u < cnt;
            const k6u32x2 w = {(unsigned)__float_as_int(live ? p : -INFINITY), live ? v[u][1] : 0u};
            *(k6u32x2*)(LB + (p0 + u) * 8) = w;
            if (!VEX && live) mn = fminf(mn, nxx[v[u][1] & 4095u]);
        }
    }
    cnts[qs * Cut::NL + t] = cnt;
    lmn[qs * Cut::NL + t] = mn;
}

// The canonical distance of (query row q, candidate row j) of the cloud at xb: dot = fmaf chain over the channels ascending from +0,
// t = fl(2 dot - xx_j), pd = fl(t - xx_q) (oracle/knn_canon.c) -- this arithmetic is what makes the indices bit-exact.  xvec (16-byte
// aligned rows, C % 4 == 0): both rows fetched CHV float4 pieces at a time (2 x CHV x 16 bytes in flight per lane).
template <int CHV>
__device__ __forceinline__ float k6_canon_pd(const float* xb, int ld, int C, bool xvec, const float* xxb, int q, int j) {
    const float* rq = xb + (size_t)q * ld;
    const float* rj = xb + (size_t)j * ld;
    float acc = 0.f;
    if (!xvec) {
        for (int c = 0; c < C; ++c) acc = fmaf(rq[c], rj[c], acc);
    } else {
        for (int c = 0; c < C; c += 4 * CHV) {
            f32x4 a4[CHV], b4[CHV];
#pragma unroll
            for (int u = 0; u < CHV; ++u)
                if (c + 4 * u < C) { a4[u] = *(const f32x4*)(rq + c + 4 * u); b4[u] = *(const f32x4*)(rj + c + 4 * u); }
#pragma unroll
            for (int u = 0; u < CHV; ++u)
                if (c + 4 * u < C) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = fmaf(a4[u][e], b4[u][e], acc);
                }
        }
    }
    const float t2 = fmaf(2.0f, acc, -xxb[j]);
    return t2 - xxb[q];
}

// ------------------------------------------------------------------------------------------------------------------------------------
// The finals: exact ranks of a query's survivors.  What a wave needs for them:
struct K6Fin {
    const float *xb, *xxb, *xcb;        // the cloud: fp32 rows, canonical (raw) and centred squared norms
    int ld, C, k;
    bool xvec;                          // rows can be fetched as float4
    float xxmax, canon;                 // the cloud's largest raw norm; K6_CANON
    char* lists;                        // [512][K6_LSTR], pd domain (k6_f0)
    const int* cnts;                    // [queries of the workgroup][NL] list lengths
    const float* lmn;                   // [queries of the workgroup][NL] min of -xc_j / 2 over each list's survivors
    unsigned* wl;                       // this wave's 512 words of work space
    int* out;                           // idx rows of the cloud
    int lane, qg, part, qwg0;           // qwg0: first query of the workgroup, local to the cloud
};
// address of list t of query qlc of the wave's group
template <class Cut>
__device__ __forceinline__ char* k6_list(const K6Fin& f, int qlc, int t) { return f.lists + (size_t)(Cut::list_at(f.qg, qlc, t) * K6_LSTR); }
// query qq of the workgroup: pp[t] = survivors ahead of list t (pp[NL] = all of them), cmx = its longest list, and
// 2 E = the width of the window inside which the approximate values do not decide (error budget: file header; 0 for exact values)
template <class Cut>
__device__ __forceinline__ void k6_query_lists(const K6Fin& f, int qq, bool exact, int (&pp)[Cut::NL + 1], int& cmx, float& E2) {
    float mn = 0.f;
    pp[0] = 0;
#pragma unroll
    for (int t4 = 0; t4 < Cut::NL; t4 += 4) {
        const k6i32x4 c4 = *(const k6i32x4*)(f.cnts + qq * Cut::NL + t4);
        const f32x4 m4 = *(const f32x4*)(f.lmn + qq * Cut::NL + t4);
#pragma unroll
        for (int u = 0; u < 4; ++u) pp[t4 + u + 1] = pp[t4 + u] + c4[u];
        const int cm4 = max(max(c4[0], c4[1]), max(c4[2], c4[3]));
        const float mn4 = fminf(fminf(m4[0], m4[1]), fminf(m4[2], m4[3]));
        cmx = t4 ? max(cmx, cm4) : cm4;
        mn = t4 ? fminf(mn, mn4) : mn4;
    }
    const float xm = -2.0f * mn;                               // largest centred squared norm among the query's survivors
    const int qrow = f.qwg0 + qq;
    E2 = exact ? 0.0f : 2.0f * (K6_EPS * (f.xcb[qrow] + xm) + f.canon * (f.xxb[qrow] + f.xxmax));
}
// entry e of a query's concatenated lists: list t, position e - pb
template <int NL>
__device__ __forceinline__ void k6_locate(const int (&pp)[NL + 1], int e, int& t, int& pb) {
    t = 0; pb = 0;
#pragma unroll
    for (int u = 1; u < NL; ++u) { const bool ge = e >= pp[u]; t = ge ? u : t; pb = ge ? pp[u] : pb; }
}

// value of the same register in lane ^ D: DPP row_ror at 8, the permlane swaps at 16 / 32 (no LDS)
template <int D>
__device__ __forceinline__ unsigned k6_xlane(unsigned v, int lane) {
    if constexpr (D == 8) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xf, 0xf, true);
    else if constexpr (D == 16) { const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false); return (lane & 16) ? r[0] : r[1]; }
    else { const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false); return (lane & 32) ? r[0] : r[1]; }
}
// compare-exchange of a lane's positions a, a ^ jj; desc: the larger value to the lower position
__device__ __forceinline__ void k6_cex_local(float (&pv)[8], int (&jv)[8], int jj, bool desc) {
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int c = a ^ jj;
        if (c > a) {
            const bool sw = desc ? pv[a] < pv[c] : pv[a] > pv[c];
            const float ta = sw ? pv[c] : pv[a], tc = sw ? pv[a] : pv[c];
            const int ja = sw ? jv[c] : jv[a], jc = sw ? jv[a] : jv[c];
            pv[a] = ta; pv[c] = tc; jv[a] = ja; jv[c] = jc;
        }
    }
}
// ... of position i of this lane and of lane ^ D: the lane without bit D holds the lower position
template <int D>
__device__ __forceinline__ void k6_cex_cross(float (&pv)[8], int (&jv)[8], int lane, bool desc) {
    const bool low = (lane & D) == 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float ov = __uint_as_float(k6_xlane<D>(__float_as_uint(pv[i]), lane));
        const int oj = (int)k6_xlane<D>((unsigned)jv[i], lane);
        const bool sw = low ? (desc ? pv[i] < ov : pv[i] > ov) : (desc ? ov < pv[i] : ov > pv[i]);
        pv[i] = sw ? ov : pv[i]; jv[i] = sw ? oj : jv[i];
    }
}

// ---- fast final (every query of the wave has at most FCAP = 8 FL survivors -- the normal case): FL LANES PER QUERY.  Wave (qg, part) finishes
// queries part * FQ .. + FQ - 1 of its group; lane l serves query l % FQ and holds rank positions 8 m .. 8 m + 7 of its FCAP (m = l / FQ).  The FL lanes
// pull the query's survivors into registers and sort them by pd' with a bitonic network whose exchanges at distance >= 8 cross lanes (k6_xlane):
// with four lanes 72 compare-exchanges per lane instead of the 240 of one lane per query.  Then: the ones whose gap to a neighbour in rank is
// within 2 E are flagged, get their canonical distances (all flagged pairs of the wave packed densely over its lanes: fmaf chains over the fp32
// rows), and the flagged runs are settled with odd-even passes under the full order (value desc, index asc); the pair across a lane boundary goes
// through two shuffles.  An unflagged survivor never moves: its gaps exceed 2 E.  VEX: the lists hold exact values, only exact ties are flagged.
// Returns false, with nothing written, when a query of the wave has more survivors than that: the counting final takes the wave.
template <class Cut, int CT, bool VEX>
__device__ __forceinline__ bool k6_fast_final(const K6Fin& f) {
    constexpr int FL = Cut::FL, FQ = Cut::FQ, FCAP = Cut::FCAP, NL = Cut::NL;
    const int lane = f.lane, ql = lane & (FQ - 1), m = lane / FQ;
    const int qlc = f.part * FQ + ql;
    const int qq = f.qg * 32 + qlc, qrow = f.qwg0 + qq;
    int pp[NL + 1], cmx;
    float E2;
    k6_query_lists<Cut>(f, qq, VEX, pp, cmx, E2);
    const int n = pp[NL];
    int nmaxw = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmaxw = max(nmaxw, __shfl_xor(nmaxw, o, 64));
    if (nmaxw > FCAP) return false;
    float pv[8];
    int jv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int e = 8 * m + i;
        int t, pb;
        k6_locate<NL>(pp, e, t, pb);
        const k6u32x2 v = *(const k6u32x2*)(k6_list<Cut>(f, qlc, e < n ? t : 0) + (e < n ? e - pb : 0) * 8);
        pv[i] = e < n ? __int_as_float((int)v[0]) : -INFINITY;
        jv[i] = e < n ? (int)v[1] : 0x7fffffff;
    }
    // bitonic network over positions a = 8 m + i; a pair keeps the larger value at the lower position iff (a & k2) == 0
#pragma unroll
    for (int a = 0; a < 8; a += 2) {                            // k2 = 2
        const bool desc = (a & 2) == 0;
        const bool sw = desc ? pv[a] < pv[a + 1] : pv[a] > pv[a + 1];
        const float ta = sw ? pv[a + 1] : pv[a], tc = sw ? pv[a] : pv[a + 1];
        const int ja = sw ? jv[a + 1] : jv[a], jc = sw ? jv[a] : jv[a + 1];
        pv[a] = ta; pv[a + 1] = tc; jv[a] = ja; jv[a + 1] = jc;
    }
#pragma unroll
    for (int jj = 2; jj > 0; jj >>= 1)                          // k2 = 4: direction by bit 2 of the position
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            const int c = a ^ jj;
            if (c > a) {
                const bool desc = (a & 4) == 0;
                const bool sw = desc ? pv[a] < pv[c] : pv[a] > pv[c];
                const float ta = sw ? pv[c] : pv[a], tc = sw ? pv[a] : pv[c];
                const int ja = sw ? jv[c] : jv[a], jc = sw ? jv[a] : jv[c];
                pv[a] = ta; pv[c] = tc; jv[a] = ja; jv[c] = jc;
            }
        }
    // k2 = 8 s, s = 1 .. FL: direction by bit s of m (the last stage: descending), exchanges with lanes m ^ (s / 2) .. m ^ 1, i.e. at lane
    // distances FQ, 2 FQ, 4 FQ = 16, 32 for four lanes per query, 8, 16, 32 for eight, then inside the lane
    auto cex_lane = [&](bool d) { k6_cex_local(pv, jv, 4, d); k6_cex_local(pv, jv, 2, d); k6_cex_local(pv, jv, 1, d); };
    { const bool d = (m & 1) == 0; cex_lane(d); }                                                                                   // k2 = 8
    { const bool d = (m & 2) == 0; k6_cex_cross<FQ>(pv, jv, lane, d); cex_lane(d); }                                                // k2 = 16
    { const bool d = (m & 4) == 0; k6_cex_cross<2 * FQ>(pv, jv, lane, d); k6_cex_cross<FQ>(pv, jv, lane, d); cex_lane(d); }         // k2 = 32
    if constexpr (FL == 8) { k6_cex_cross<4 * FQ>(pv, jv, lane, true); k6_cex_cross<2 * FQ>(pv, jv, lane, true); k6_cex_cross<FQ>(pv, jv, lane, true); cex_lane(true); }   // k2 = 64
    // flag: gap to the next survivor in rank not provably larger than 2 E (dead tail entries: -inf, never flagged)
    const float nxt0 = __shfl(pv[0], lane + FQ, 64), prv7 = __shfl(pv[7], lane - FQ, 64);
    unsigned amb = 0u;
#pragma unroll
    for (int i = 0; i < 7; ++i) amb |= (8 * m + i + 1 < n && !(pv[i] - pv[i + 1] > E2)) ? (3u << i) : 0u;
    amb |= (m < FL - 1 && 8 * m + 8 < n && !(pv[7] - nxt0 > E2)) ? 0x80u : 0u;
    amb |= (m > 0 && 8 * m < n && !(prv7 - pv[0] > E2)) ? 1u : 0u;
    const int nfl = __builtin_popcount(amb);                   // this lane's flagged entries; the query's: the FL lanes' sum
    int nflag = 0, foff = 0;
#pragma unroll
    for (int t = 0; t < FL; ++t) { const int fl = __shfl(nfl, ql + FQ * t, 64); nflag += fl; foff += t < m ? fl : 0; }
    unsigned* slots = f.wl + ql * FCAP + foff;                 // this lane's part of the query's [FCAP]: candidate index in, canonical distance out
    {
        int c = 0;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            if ((amb >> a) & 1u) { slots[c] = (unsigned)jv[a]; ++c; }
        }
    }
    int fmaxw = nflag;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fmaxw = max(fmaxw, __shfl_xor(fmaxw, o, 64));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // Canonical distances of the flagged pairs, DENSELY packed over the wave's lanes: pair i of the wave = (query, slot) by a prefix sum of
    // the FQ queries' flag counts (the counts differ a lot from query to query: slot-by-slot rounds ran at a third of the lanes).  Both rows
    // fetched whole (2 x 16 x 16 bytes in flight per lane at C = 64; 8 pieces at C = 128: register budget), fmaf chain channels ascending.
    // (Staging the rows through LDS with cooperative, fully coalesced fetches was built and measured: 2x slower -- the phase is bound by its
    // chain of dependent steps, not by cache-line transactions.)
    if (fmaxw > 0) {
        int offs[FQ + 1];
        offs[0] = 0;
#pragma unroll
        for (int q = 0; q < FQ; ++q) offs[q + 1] = offs[q] + __builtin_amdgcn_readlane(nflag, q);      // (scalar)
        const int total = offs[FQ];
        const int qbase = f.qwg0 + f.qg * 32 + f.part * FQ;
        for (int i0 = 0; i0 < total; i0 += 64) {
            const int i = i0 + lane;
            if (i < total) {
                int q = 0, ob = 0;
#pragma unroll
                for (int t = 1; t < FQ; ++t) { const bool ge = i >= offs[t]; q = ge ? t : q; ob = ge ? offs[t] : ob; }
                unsigned* sp = f.wl + q * FCAP + (i - ob);
                const int j = (int)*sp;
                *sp = (unsigned)__float_as_int(k6_canon_pd<CT >= 128 ? 8 : 16>(f.xb, f.ld, f.C, f.xvec, f.xxb, qbase + q, j));
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    {
        int c = 0;
#pragma unroll
        for (int a = 0; a < 8; ++a) {
            if ((amb >> a) & 1u) { pv[a] = __int_as_float((int)slots[c]); ++c; }
        }
    }
    // settle the flagged runs: odd-even transposition passes under the full order until nothing moves (a run of r entries needs <= r passes)
    if (fmaxw > 0) {
        for (int pass = 0; pass < FCAP; ++pass) {
            bool moved = false;
#pragma unroll
            for (int par = 0; par < 2; ++par)                   // positions (8 m + a, + 1) inside the lane: a even, then a odd
#pragma unroll
                for (int a = par; a < 7; a += 2) {
                    const bool sw = k6_beats(pv[a + 1], jv[a + 1], pv[a], jv[a]);
                    const float ta = sw ? pv[a + 1] : pv[a], tc = sw ? pv[a] : pv[a + 1];
                    const int ja = sw ? jv[a + 1] : jv[a], jc = sw ? jv[a] : jv[a + 1];
                    pv[a] = ta; pv[a + 1] = tc; jv[a] = ja; jv[a + 1] = jc;
                    moved |= sw;
                }
            {                                                    // the odd pair across the lane boundary: (8 m + 7, 8 (m + 1))
                const float nv = __shfl(pv[0], lane + FQ, 64), pvv = __shfl(pv[7], lane - FQ, 64);
                const int nj = __shfl(jv[0], lane + FQ, 64), pj = __shfl(jv[7], lane - FQ, 64);
                const bool swh = m < FL - 1 && k6_beats(nv, nj, pv[7], jv[7]);      // the next lane's first entry beats my last one
                const bool swl = m > 0 && k6_beats(pv[0], jv[0], pvv, pj);          // my first entry beats the previous lane's last one
                pv[7] = swh ? nv : pv[7]; jv[7] = swh ? nj : jv[7];
                pv[0] = swl ? pvv : pv[0]; jv[0] = swl ? pj : jv[0];
                moved |= swh | swl;
            }
            if (!__any(moved)) break;
        }
    }
    int* out = f.out + (size_t)qrow * f.k;
#pragma unroll
    for (int a = 0; a < 8; ++a) {
        const int pos = 8 * m + a;
        if (pos < f.k && pos < n) out[pos] = jv[a];
    }
    return true;
}

// flush of the counting final: canonical distance of every pair on the wave's work list (items: entry offset / 8 | query of the
// workgroup << 16) back into the lists, then a recount of those entries under the full order (value desc, index asc)
template <class Cut>
__device__ __forceinline__ void k6_flush(const K6Fin& f, int wcnt) {
    constexpr int RU = Cut::NL == 4 ? 4 : 1;                   // lists per trip of the recount (eight lists stay a loop: 192 unrolled comparisons are only code size)
    const int lane = f.lane;
    for (int i0 = 0; i0 < wcnt; i0 += 64) {
        const int i = i0 + lane;
        if (i < wcnt) {
            const unsigned item = f.wl[i];
            char* ent = f.lists + (size_t)(item & 0xffffu) * 8;
            const int j = *(const int*)(ent + 4);
            *(float*)ent = k6_canon_pd<8>(f.xb, f.ld, f.C, f.xvec, f.xxb, f.qwg0 + (int)(item >> 16), j);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int i0 = 0; i0 < wcnt; i0 += 64) {
        const int i = i0 + lane;
        const bool on = i < wcnt;
        const unsigned item = on ? f.wl[i] : 0u;
        const int qq_ = (int)(item >> 16), qlc_ = qq_ & 31;
        const k6u32x2 me = *(const k6u32x2*)(f.lists + (size_t)(item & 0xffffu) * 8);
        const float pm = __int_as_float((int)me[0]);
        const int jm = (int)me[1];
        int rank = 0;
#pragma unroll RU
        for (int t = 0; t < Cut::NL; ++t) {
            const char* L = k6_list<Cut>(f, qlc_, t);
#pragma unroll
            for (int p0 = 0; p0 < K6_CAP; p0 += 8) {
                k6u32x2 ke[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) ke[u] = *(const k6u32x2*)(L + (p0 + u) * 8);
#pragma unroll
                for (int u = 0; u < 8; ++u) rank += k6_beats(__int_as_float((int)ke[u][0]), (int)ke[u][1], pm, jm) ? 1 : 0;
            }
        }
        if (on && rank < f.k) f.out[(size_t)(f.qwg0 + qq_) * f.k + rank] = jm;
    }
}

// ---- counting final (a query of the wave has more than FCAP survivors, or the lists are exact): rank by counting, two queries per trip (one
// per half-wave); lane l31 owns entries l31 + 32 s of the query's NL concatenated lists.  Per entry of the query: rank += (pd'_e > mine),
// near += (|pd'_e - mine| <= 2 E).  near > 1 (I count myself): AMBIGUOUS -> the wave's work list; everyone else is written out at once.
// `exact` values: 2 E = 0, only exact ties go through the flush's full-order recount.
template <class Cut>
__device__ __forceinline__ void k6_counting_final(const K6Fin& f, bool exact) {
    constexpr int NL = Cut::NL, FQ = Cut::FQ;
    constexpr int PU = NL == 4 ? 4 : 1;                        // list positions per trip of the counting loop: 4 x 4 lists, 1 x 8 lists
    const int lane = f.lane, l31 = lane & 31, h = lane >> 5;
    int wcnt = 0;                                              // wave-uniform
    for (int it = 0; it < FQ / 2; ++it) {
        const int qlc = f.part * FQ + it * 2 + h;              // query of the group
        const int qq = f.qg * 32 + qlc;                        // query of the workgroup
        int pp[NL + 1], cmx;
        float E2;
        k6_query_lists<Cut>(f, qq, exact, pp, cmx, E2);
        const int n = pp[NL];
        const int nmax = max(__builtin_amdgcn_readlane(n, 0), __builtin_amdgcn_readlane(n, 32));
        cmx = max(__builtin_amdgcn_readlane(cmx, 0), __builtin_amdgcn_readlane(cmx, 32));
        for (int s0 = 0; s0 < nmax; s0 += 32) {                // one trip unless a query has more than 32 survivors
            const int e = s0 + l31;
            const bool valid = e < n;
            int t, pb;
            k6_locate<NL>(pp, e, t, pb);
            const char* mine = k6_list<Cut>(f, qlc, valid ? t : 0) + (valid ? e - pb : 0) * 8;
            const k6u32x2 me = *(const k6u32x2*)mine;
            const float pm = __int_as_float((int)me[0]);
            const int j = (int)me[1];
            int rank = 0, near = 0;
            for (int p0 = 0; p0 < cmx; p0 += PU) {             // (the lists are filled to K6_LENT with -inf: whole trips, unmasked)
#pragma unroll
                for (int u = 0; u < PU; ++u)
#pragma unroll
                    for (int lt = 0; lt < NL; ++lt) {
                        const float a = *(const float*)(k6_list<Cut>(f, qlc, lt) + (p0 + u) * 8);
                        rank += a > pm ? 1 : 0;
                        near += fabsf(a - pm) <= E2 ? 1 : 0;
                    }
            }
            const bool amb = valid && !(near <= 1);            // another survivor inside my 2 E window (I count once myself)
            if (valid && !amb && rank < f.k) f.out[(size_t)(f.qwg0 + qq) * f.k + rank] = j;
            const unsigned long long mk = __ballot(amb);
            if (mk) {
                const int before = __builtin_popcountll(mk & ((1ull << lane) - 1ull));
                if (amb) f.wl[wcnt + before] = (unsigned)((mine - f.lists) >> 3) | ((unsigned)qq << 16);
                wcnt += __builtin_popcountll(mk);
            }
        }
        if (wcnt > 512 - 2 * NL * K6_CAP || (it == FQ / 2 - 1 && wcnt > 0)) {       // (a trip adds at most 2 x NL x K6_CAP items)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            k6_flush<Cut>(f, wcnt);
            wcnt = 0;
        }
    }
}

// Workgroup = 8 waves = 128 queries x all N candidates of their cloud.  Wave w: qg = w & 3 picks a group of 32 queries, ch = w >> 2 the
// half of the candidates it sweeps: two waves per SIMD (the selection phases are vector-issue bound, and a lone wave issues at half rate),
// no barrier inside a sweep.  (Two query groups per wave against the same fragments -- half the fragment traffic -- was built and measured:
// the sweeps gain 10 %, every selection phase loses 2x at one wave per SIMD.)
// Measured (B = 32, N = 1024, k = 20): 37.7 us per call against 41.5 on knn_mfma5_kernel<4>; clock stamps between the phases (clocks per
// workgroup): pass A 11.7 k, pass B 24.7 k, tau 5.5 k, final 11.4 k of 64 k -- the sweeps are LDS-issue bound, not vector bound: every
// ds_read_b128 of a candidate row serves 64 (query, candidate) pairs whatever the arithmetic (16 reads per tile and wave, 8 waves), and
// the masked survivor append doubles that in pass B.  Going below needs several queries per lane against one candidate read (another
// wave <-> query map, i.e. another list layout): not built.
// VEX (C <= 3, N <= 1024): `planes` is the {x0, x1, x2, xx} array of knn6_prep_vex_kernel; the cloud's 16 KB of it are staged in LDS (in the
// final's work-list area, dead until then) and the two sweeps are plain vector code: three FMAs, the two norm terms -- the canonical value,
// bit for bit -- per pair.  Lists hold exact distances (E = 0): the final flags only exact ties, which the full order settles by index.
template <int CT, bool VEX = false>
__global__ __launch_bounds__(512) void knn6_kernel(const float* __restrict__ x, int ld, const float* __restrict__ xx_all, const float* __restrict__ xc_all,
                                                   const char* __restrict__ planes, int N, int C, int k, int* __restrict__ idx, int B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    typedef K6Narrow Cut;
    constexpr int NKB = CT / 16;                              // 16-channel blocks = bf16 MFMA K steps per tile
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);         // (scalar: addresses below stay in SGPRs)
    const int l31 = lane & 31, h = lane >> 5, qg = wave & (Cut::QG - 1), ch = wave >> Cut::QGS;
    int b, chunk;
    xcd_cloud_map(blockIdx.x, N / Cut::QWG, B, b, chunk);
    const float* xxb = xx_all + (size_t)b * N;                // canonical squared norms (raw coordinates)
    const float* xcb = xc_all + (size_t)b * N;                // squared norms relative to the cloud's first point (the sweeps' coordinates)
    const size_t T0 = (size_t)b * (N / 32);                  // first 32-point tile of this cloud in the fragment-major image
    const float* xb = x + (size_t)b * N * ld;
    const int nt2 = N / (32 * Cut::PARTS);                    // 32-candidate tiles of this wave's half

    char* lists = (char*)sm;                                  // [512 lists][K6_LSTR]; list = Cut::list_at(qg, query of the group, 2 ch + h)
    float* xch = sm;                                          // tau exchange image [128 queries][Cut::XS], dead before pass B
    float* nxx = (float*)(lists + 512 * K6_LSTR);             // [N]  -xc_j / 2
    float* tauv = nxx + N;                                    // [128]
    int* cnts = (int*)(tauv + 128);                           // [128 queries][4 lists]
    float* red = (float*)(cnts + 512);                        // [16]
    unsigned* wlbase = (unsigned*)(red + 16);                 // [8 waves][512 words]: fast final: [16 queries][32] candidate / exact value of the ambiguous; slow final: work list
    float* lmn = (float*)(wlbase + 8 * 512);                  // [128 queries][4 lists] min of -xc_j / 2 over the list's survivors
    const unsigned lds0 = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)sm);       // LDS byte address of `lists`

    float xcmax, xxmax;
    {
        float m = 0.f, mr = 0.f;
        if (VEX) {                                            // (a NaN norm becomes an infinite bound: k6_fill_nxx)
            const f32x4* cg = (const f32x4*)planes + (size_t)b * N;
            f32x4* cl = (f32x4*)wlbase;                       // the cloud {x, xx}: the final's work lists live here later
            for (int j = tid; j < N; j += 512) { const f32x4 v = cg[j]; cl[j] = v; mr = fmaxf(mr, v[3] == v[3] ? v[3] : INFINITY); }
        } else
            k6_fill_nxx(tid, N, xcb, xxb, nxx, m, mr);
        k6_reduce_bounds(lane, wave, m, mr, red, xcmax, xxmax);
    }
    // |pd' - pd_canonical| <= K6_EPS (xc_q + xc_j)  [split products on the centred coordinates, header]
    //                        + K6_CANON (xx_q + xx_j)  [the canonical value's own distance from -|x_q - x_j|^2: an fmaf chain of C terms, the two
    //                          norms and two more roundings on the RAW coordinates: < (C + 4) 2^-23 (xx_q + xx_j)]
    const float K6_CANON = (float)(C + 4) * 1.1920929e-07f;
    const int q0 = chunk * Cut::QWG + qg * 32;                // first query of this wave's group, local to the cloud
    const float xxq = xxb[q0 + l31];                          // raw (exact path, canonical bound)
    const float xcq = VEX ? 0.f : xcb[q0 + l31];              // centred (sweeps)
    // VEX: the lists hold the canonical values themselves -- no error to budget; a non-finite norm still asks for the exact path
    const float Eq = VEX ? (xxmax < INFINITY ? 0.f : INFINITY) : K6_EPS * (xcq + xcmax) + K6_CANON * (xxq + xxmax);

    // ---------------------------------------------------------------------------------------------------------------- approximate sweeps
    k6bf16x8 qh[NKB], ql[NKB];
    f32x4 qv = {0.f, 0.f, 0.f, 0.f};                          // VEX: this lane's query {x0, x1, x2, xx}
    if constexpr (VEX) qv = ((const f32x4*)wlbase)[q0 + l31];
    const unsigned voff = (unsigned)(h * 512 + l31 * 16);     // this lane's 16 bytes inside a fragment KiB
    if constexpr (!VEX) k6_load_query<NKB>(planes, T0 + (q0 >> 5), voff, qh, ql);
    const char* cand0 = planes + (T0 + (size_t)ch * nt2) * (NKB * 2048);     // (uniform) first tile of this wave's half
    auto sweep = [&](auto&& sel) {
        if constexpr (VEX) {
            // vector sweep: acc[r] = the CANONICAL distance of (query l31, candidate (r & 3) + 8 (r >> 2) + 4 h of the tile): dot = fmaf chain
            // over the channels from +0, t = fl(2 dot - xx_j), pd = fl(t - xx_i) (oracle/knn_canon.c).  The 32 lanes of a half read the same
            // candidate: one LDS broadcast per row.
            const f32x4* cl = (const f32x4*)wlbase;
            for (int tl = 0; tl < nt2; ++tl) {
                const f32x4* cp = cl + (ch * nt2 + tl) * 32 + 4 * h;
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const f32x4 c = cp[(r & 3) + 8 * (r >> 2)];
                    float d = fmaf(qv[0], c[0], 0.f);
                    d = fmaf(qv[1], c[1], d);
                    d = fmaf(qv[2], c[2], d);
                    acc[r] = fmaf(2.0f, d, -c[3]) - qv[3];
                }
                sel(acc, tl);
            }
        } else
            k6_sweep<NKB>(cand0, voff, nxx, ch, h, nt2, qh, ql, sel);
    };

    // ---- pass A: 16 running maxima per lane (acc domain: a = dot' - xc_j / 2 is monotone in the distance for a fixed query)
    {
        float cm[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) cm[r] = -INFINITY;
        sweep([&](const f32x16& acc, int) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cm[r] = fmaxf(cm[r], acc[r]);
        });
        k6_store_maxima(xch + (qg * 32 + l31) * Cut::XS + (ch * 2 + h) * 16, cm);
    }
    __syncthreads();
    // tau = k-th largest of a query's 64 maxima: one lane per query (the ch = 0 wave of a group: one wave per SIMD; lanes 32-63 mirror), bitonic
    // network in registers
    if (ch == 0) {
        const int qs = qg * 32 + l31;
        float v[64];
        const float* src = xch + qs * Cut::XS;
#pragma unroll
        for (int i4 = 0; i4 < 16; ++i4) {
            const f32x4 t = *(const f32x4*)(src + 4 * i4);
            v[4 * i4] = t[0]; v[4 * i4 + 1] = t[1]; v[4 * i4 + 2] = t[2]; v[4 * i4 + 3] = t[3];
        }
        k6_sort64(v);
        float t = v[0];
#pragma unroll
        for (int i = 1; i < Cut::KMAX; ++i) t = (i == k - 1) ? v[i] : t;
        if (lane < 32) tauv[qs] = t;
    }
    __syncthreads();                                          // tau complete; the exchange image (aliases the lists) is dead from here on
    float thr = tauv[qg * 32 + l31] - Eq;                     // acc domain: pd' >= tau_pd - 2 E  <=>  a >= a_tau - E
    thr = thr == thr ? thr : -INFINITY;                       // (a non-finite bound Eq sends the workgroup through the exact path: `ovf` below)

    // ---- pass B: survivors -> this lane's private list (acc-domain value, candidate index): k6_append16
    const int lid = Cut::list_at(qg, l31, ch * 2 + h);
    char* LB = lists + (size_t)(lid * K6_LSTR);
    const unsigned base = lds0 + (unsigned)(lid * K6_LSTR);
    unsigned ad = base, top = base;
    sweep([&](const f32x16& acc, int tl) { k6_append16(ad, top, base, acc, thr, (ch * nt2 + tl) * 32 + 4 * h); });
    int cnt = (int)(ad - base) >> 3;
    // overflow (massive ties), or no usable bound: a non-finite norm in the cloud (the approximate values of a NaN row are NaN and survive
    // no comparison, so they would not overflow anything: ask for the exact path outright)
    const int ovf = (top > base + K6_CAP * 8 || !(Eq < INFINITY)) ? 1 : 0;
    bool exact_lists = false;
    if (__syncthreads_or(ovf)) {
        // ------------------------------------------------------------------------------------------------------------ exact path (rare)
        // f32 MFMA tiles straight from the fp32 rows (same transposed layout; the MFMA chain is the canonical fmaf chain, channels
        // ascending), every lane keeps the exact top-K6_KMAX of ITS quarter of the candidates in a sorted register list.
        const bool vec = (ld & 3) == 0 && (((uintptr_t)x) & 15) == 0 && (C & 3) == 0;
        // fragment of 32 channels [c0, c0 + 32) of a row for the f32 MFMA: f[s] = row[c0 + 2 s + h], zero beyond C (16 K-steps of 2 channels)
        auto load_frag = [&](const float* row, int c0, float (&f)[16]) {
            if (vec) {
#pragma unroll
                for (int m4 = 0; m4 < 8; ++m4) {
                    f32x4 v = {0.f, 0.f, 0.f, 0.f};
                    if (c0 + 4 * m4 < C) v = *(const f32x4*)(row + c0 + 4 * m4);
                    f[2 * m4] = h ? v[1] : v[0];
                    f[2 * m4 + 1] = h ? v[3] : v[2];
                }
            } else {
#pragma unroll
                for (int s_ = 0; s_ < 16; ++s_) f[s_] = (c0 + 2 * s_ + h < C) ? row[c0 + 2 * s_ + h] : 0.f;
            }
        };
        const float* qrowp = xb + (size_t)(q0 + l31) * ld;
        float tv[K6_KMAX];
        int ti[K6_KMAX];
#pragma unroll
        for (int s_ = 0; s_ < K6_KMAX; ++s_) { tv[s_] = -INFINITY; ti[s_] = 0x7fffffff; }
        for (int tl = 0; tl < nt2; ++tl) {
            const int j0 = (ch * nt2 + tl) * 32;
            const float* crowp = xb + (size_t)(j0 + l31) * ld;
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            for (int c0 = 0; c0 < C; c0 += 32) {               // channels ascending: the canonical chain (query fragments re-read: rare path)
                float ca[16], qa[16];
                load_frag(crowp, c0, ca);
                load_frag(qrowp, c0, qa);
#pragma unroll
                for (int s_ = 0; s_ < 16; ++s_) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s_], qa[s_], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int j = j0 + 4 * h + (r & 3) + 8 * (r >> 2);
                const float xxj = xxb[j];                                    // canonical norm of the raw row
                const float pd = fmaf(2.0f, acc[r], -xxj) - xxq;
                if (k6_beats(pd, j, tv[K6_KMAX - 1], ti[K6_KMAX - 1])) {
                    bool bs[K6_KMAX];
#pragma unroll
                    for (int s_ = 0; s_ < K6_KMAX; ++s_) bs[s_] = k6_beats(pd, j, tv[s_], ti[s_]);
#pragma unroll
                    for (int s_ = K6_KMAX - 1; s_ > 0; --s_) {
                        tv[s_] = bs[s_ - 1] ? tv[s_ - 1] : (bs[s_] ? pd : tv[s_]);
                        ti[s_] = bs[s_ - 1] ? ti[s_ - 1] : (bs[s_] ? j : ti[s_]);
                    }
                    tv[0] = bs[0] ? pd : tv[0];
                    ti[0] = bs[0] ? j : ti[0];
                }
            }
        }
        cnt = 0;
#pragma unroll
        for (int s_ = 0; s_ < K6_KMAX; ++s_) {
            if (s_ < k && ti[s_] != 0x7fffffff) {
                const k6u32x2 e = {(unsigned)__float_as_int(tv[s_]), (unsigned)ti[s_]};
                *(k6u32x2*)(LB + s_ * 8) = e;
                cnt = s_ + 1;
            }
        }
        exact_lists = true;
    }
    k6_f0<Cut, VEX>(LB, cnt, exact_lists, xcq, nxx, cnts, lmn, qg * 32 + l31, ch * 2 + h);          // lists -> pd domain
    __syncthreads();

    // ---------------------------------------------------------------------------------------------------------------- final: exact ranks
    const bool xvec = (ld & 3) == 0 && (((uintptr_t)x) & 15) == 0 && (C & 3) == 0;
    const K6Fin fin = {xb, xxb, xcb, ld, C, k, xvec, xxmax, K6_CANON, lists, cnts, lmn, wlbase + wave * 512, idx + (size_t)b * N * k,
                       lane, qg, ch, chunk * Cut::QWG};
    if (!exact_lists && k6_fast_final<Cut, CT, VEX>(fin)) return;
    k6_counting_final<Cut>(fin, exact_lists || VEX);
}

// ------------------------------------------------------------------------------------------------------------------------------------
// v6 WIDE (24 < k <= 40, N % 128 == 0, C <= 128): PointSegDA's graphs (k = 40, PointSegDA/Models.py:6-15; BASELINE.json configs[4]).
// The phases of knn6_kernel (the k6_* functions above) under the other cut of the workgroup, K6Wide, so that the 232-byte survivor lists
// still fit the CU:
//   * workgroup = 64 queries (two groups of 32) x all N candidates; wave w: qg = w & 1, ch = w >> 1 sweeps a QUARTER of the candidates.
//     A query's candidates are cut into 8 sub-ranges (quarter x half-wave lane): 512 lists of K6_CAP = 24 entries as before, but a query
//     now owns 8 of them.  With k = 40 a query keeps ~50 survivors, ~6 per list: K6_CAP is six standard deviations away.
//   * pass A leaves 128 running maxima per query; tau = their k-th largest.  Two lanes per query sort 64 each (k6_sort64),
//     exchange them through v_permlane32_swap (max(a[i], b[63 - i]) = the 64 largest of the union, a bitonic sequence) and
//     merge.  Against 64 maxima the bound is tighter: ~1.2 k survivors instead of ~1.6 k.
//   * fast final: EIGHT lanes per query (64 rank positions; exchanges at lane distance 8 through DPP row_ror, 16 / 32 through the
//     permlane swaps); the counting final takes queries with more than 64 survivors.
//   * no exact path inside: a workgroup whose lists overflow (massive ties: padded clouds) or whose bound is not finite raises its CLOUD's
//     flag and leaves; the v5 kernel (knn.hip, KB = 1) runs right behind on the flagged clouds only (its workgroups of other clouds return at
//     once) and overwrites their rows.  Indices bit-exact either way: both kernels rank by the canonical distance under the same total order.
template <int CT>
__global__ __launch_bounds__(512) void knn6w_kernel(const float* __restrict__ x, int ld, const float* __restrict__ xx_all, const float* __restrict__ xc_all,
                                                    const char* __restrict__ planes, int N, int C, int k, int* __restrict__ idx, int B,
                                                    int* __restrict__ cloud_flag) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    typedef K6Wide Cut;
    constexpr int NKB = CT / 16;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5, qg = wave & (Cut::QG - 1), ch = wave >> Cut::QGS;
    int b, chunk;
    xcd_cloud_map(blockIdx.x, N / Cut::QWG, B, b, chunk);
    const float* xxb = xx_all + (size_t)b * N;
    const float* xcb = xc_all + (size_t)b * N;
    const size_t T0 = (size_t)b * (N / 32);
    const float* xb = x + (size_t)b * N * ld;
    const int nt4 = N / (32 * Cut::PARTS);                    // 32-candidate tiles of this wave's quarter

    char* lists = (char*)sm;                                  // [512 lists][K6_LSTR]; list = Cut::list_at(qg, query of the group, 2 ch + h)
    float* xch = sm;                                          // tau exchange image [64 queries][Cut::XS], dead before pass B
    float* nxx = (float*)(lists + 512 * K6_LSTR);             // [N]  -xc_j / 2
    float* tauv = nxx + N;                                    // [64] (+64 unused)
    int* cnts = (int*)(tauv + 128);                           // [64 queries][8 lists]
    float* red = (float*)(cnts + 512);                        // [16]
    unsigned* wlbase = (unsigned*)(red + 16);                 // [8 waves][512 words]: fast final [8 queries][64]; counting final: work list
    float* lmn = (float*)(wlbase + 8 * 512);                  // [64 queries][8 lists]
    const unsigned lds0 = (unsigned)(unsigned long)((__attribute__((address_space(3))) char*)sm);

    float xcmax, xxmax;
    {
        float m = 0.f, mr = 0.f;
        k6_fill_nxx(tid, N, xcb, xxb, nxx, m, mr);
        k6_reduce_bounds(lane, wave, m, mr, red, xcmax, xxmax);
    }
    const float K6_CANON = (float)(C + 4) * 1.1920929e-07f;
    const int q0 = chunk * Cut::QWG + qg * 32;                // first query of this wave's group, local to the cloud
    const float xxq = xxb[q0 + l31];
    const float xcq = xcb[q0 + l31];
    const float Eq = K6_EPS * (xcq + xcmax) + K6_CANON * (xxq + xxmax);      // (error budget: the file header)

    k6bf16x8 qh[NKB], ql[NKB];
    const unsigned voff = (unsigned)(h * 512 + l31 * 16);
    k6_load_query<NKB>(planes, T0 + (q0 >> 5), voff, qh, ql);
    const char* cand0 = planes + (T0 + (size_t)ch * nt4) * (NKB * 2048);

    // ---- pass A: 16 running maxima per lane -> 128 per query
    {
        float cm[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) cm[r] = -INFINITY;
        k6_sweep<NKB>(cand0, voff, nxx, ch, h, nt4, qh, ql, [&](const f32x16& acc, int) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cm[r] = fmaxf(cm[r], acc[r]);
        });
        k6_store_maxima(xch + (qg * 32 + l31) * Cut::XS + (ch * 2 + h) * 16, cm);
    }
    __syncthreads();
    // tau = k-th largest of the query's 128 maxima: lanes (l31, h = 0 / 1) of the group's ch = 0 wave each sort 64, then merge
    if (ch == 0) {
        const int qs = qg * 32 + l31;
        float v[64];
        const float* src = xch + qs * Cut::XS + h * 64;
#pragma unroll
        for (int i4 = 0; i4 < 16; ++i4) {
            const f32x4 t = *(const f32x4*)(src + 4 * i4);
            v[4 * i4] = t[0]; v[4 * i4 + 1] = t[1]; v[4 * i4 + 2] = t[2]; v[4 * i4 + 3] = t[3];
        }
        k6_sort64(v);
        // the 64 largest of the two sorted halves: w[i] = max(mine[i], other[63 - i]) (a bitonic sequence; the partner lane holds it reversed)
        float w[64];
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[63 - i]), __float_as_uint(v[63 - i]), false, false);
            w[i] = fmaxf(v[i], __uint_as_float(h ? r[0] : r[1]));
        }
#pragma unroll
        for (int j = 32; j > 0; j >>= 1)
#pragma unroll
            for (int i = 0; i < 64; ++i) {
                const int l = i ^ j;
                if (l > i) { const float lo = fminf(w[i], w[l]), hi = fmaxf(w[i], w[l]); w[i] = hi; w[l] = lo; }
            }
        float t = w[0];
#pragma unroll
        for (int i = 1; i < Cut::KMAX; ++i) t = (i == k - 1) ? w[i] : t;
        if (lane < 32) tauv[qs] = t;
    }
    __syncthreads();                                          // tau complete; the exchange image (aliases the lists) is dead from here on
    float thr = tauv[qg * 32 + l31] - Eq;
    thr = thr == thr ? thr : -INFINITY;

    // ---- pass B: survivors -> this lane's private list
    const int lid = Cut::list_at(qg, l31, ch * 2 + h);
    char* LB = lists + (size_t)lid * K6_LSTR;
    const unsigned base = lds0 + (unsigned)(lid * K6_LSTR);
    unsigned ad = base, top = base;
    k6_sweep<NKB>(cand0, voff, nxx, ch, h, nt4, qh, ql, [&](const f32x16& acc, int tl) { k6_append16(ad, top, base, acc, thr, (ch * nt4 + tl) * 32 + 4 * h); });
    const int cnt = (int)(ad - base) >> 3;
    const int ovf = (top > base + K6_CAP * 8 || !(Eq < INFINITY)) ? 1 : 0;
    if (__syncthreads_or(ovf)) {                              // overflow / no usable bound: this cloud goes to the v5 kernel launched behind
        if (tid == 0) cloud_flag[b] = 1;
        return;
    }
    k6_f0<Cut, false>(LB, cnt, false, xcq, nxx, cnts, lmn, qg * 32 + l31, ch * 2 + h);              // lists -> pd domain
    __syncthreads();

    // ---------------------------------------------------------------------------------------------------------------- final: exact ranks
    const bool xvec = (ld & 3) == 0 && (((uintptr_t)x) & 15) == 0 && (C & 3) == 0;
    const K6Fin fin = {xb, xxb, xcb, ld, C, k, xvec, xxmax, K6_CANON, lists, cnts, lmn, wlbase + wave * 512, idx + (size_t)b * N * k,
                       lane, qg, ch, chunk * Cut::QWG};
    if (k6_fast_final<Cut, CT, false>(fin)) return;
    k6_counting_final<Cut>(fin, false);
}

template <int CT>
static int knn6_go(hipStream_t st, const KnnPlan& p, bool wide, const float* x, int ld, int B, int N, int C, int k, int* idx, float* xx, float* xc, char* planes,
                   int* flags) {
    const int P = B * N;
    const dim3 grid(p.grid_x), block(p.block);
    hipLaunchKernelGGL((knn6_prep_kernel<CT>), dim3((P + 255) / 256), dim3(256), 0, st, x, ld, P, N, C, xx, xc, planes, idx, k, flags);
    if (wide) return mlsp_launch_lds(st, knn6w_kernel<CT>, grid, block, p.lds, x, ld, xx, xc, planes, N, C, k, idx, B, flags);
    return mlsp_launch_lds(st, knn6_kernel<CT>, grid, block, p.lds, x, ld, xx, xc, planes, N, C, k, idx, B);
}

// The v6 families of a plan (knn_plan.h: VEX, V6, V6W_V5): the prep kernel, then the search kernel.  xx [B*N] floats and `planes` (the
// plan's plane_bytes) are workspace that the launch writes (xx = canonical squared norms, as sqnorm_kernel).  V6W_V5: *flags_out = the
// per-cloud flags ([B] ints inside `planes`) the caller hands to the v5 launch behind it.  The kernels' own preconditions are checked here.
int launch_knn6(hipStream_t st, const KnnPlan& p, const float* x, int ld, int B, int N, int C, int k, int* idx, float* xx, void* planes,
                int** flags_out) {
    const bool vex = p.family == KNN_FAM_VEX, wide = p.family == KNN_FAM_V6W_V5;
    const bool takes = vex ? knn6_vex_supported(B, N, C, k) : wide ? knn6w_supported(B, N, C, k) : p.family == KNN_FAM_V6 && knn6_supported(B, N, C, k);
    if (p.status != MLSP_OK || !takes || !planes || (((uintptr_t)planes) & 15)) return MLSP_ERR_UNSUPPORTED;
    const int P = B * N;
    if (vex) {
        hipLaunchKernelGGL(knn6_prep_vex_kernel, dim3((P + 255) / 256), dim3(256), 0, st, x, ld, P, C, xx, (f32x4*)planes, idx, k);
        return mlsp_launch_lds(st, knn6_kernel<16, true>, dim3(p.grid_x), dim3(p.block), p.lds, x, ld, xx, xx, (const char*)planes, N, C, k, idx, B);
    }
    float* xc = (float*)((char*)planes + (size_t)P * p.CT * 4);              // centred norms behind the fragment image (knn6_plane_bytes covers them)
    int* flags = wide ? (int*)(xc + (size_t)P) : nullptr;
    *flags_out = flags;
    if (p.CT == 16) return knn6_go<16>(st, p, wide, x, ld, B, N, C, k, idx, xx, xc, (char*)planes, flags);
    if (p.CT == 64) return knn6_go<64>(st, p, wide, x, ld, B, N, C, k, idx, xx, xc, (char*)planes, flags);
    return knn6_go<128>(st, p, wide, x, ld, B, N, C, k, idx, xx, xc, (char*)planes, flags);
}
