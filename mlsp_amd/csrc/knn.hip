// Brute-force self-kNN in canonical arithmetic + the reverse (transposed) neighbour index.
// Replaces PointDA/model_utils.py:9-16 `knn` (and its PointSegDA/Models.py:8-15 twin).  The
// [B,N,N] distance matrix of the reference never exists: distances live in registers only.
//
// Canonical arithmetic (bit-exact twin of oracle/knn_canon.c):
//   dot(i,j) = fmaf chain over c ascending from +0;  xx(j) = same chain on (x_j,x_j)
//   pd(i,j)  = fl( fl(2*dot - xx(j)) - xx(i) );  order = pd descending, ties -> lower j.
//
// v1 structure: one query per lane, 4 waves per workgroup share 64 queries and each scans a quarter
// of the candidates (staged through LDS, read as wave-uniform broadcasts); each lane keeps a sorted
// top-K list in registers; the 4 partial lists are merged through LDS under the same total order,
// so the result does not depend on the partition.
#include "common.h"
#include <type_traits>
#include <math.h>
#include <cstdlib>

#define KNN_QB 64      // queries per workgroup
#define KNN_TJ 32      // candidates per LDS tile per wave

// squared norms with the canonical chain
// `idx` (nullable): the kNN output [P][k], zero-filled here -- a row with fewer than k comparable candidates (NaN coordinates) keeps index 0
// in the positions the selection kernels never write, as oracle/knn_canon.c does; no gather downstream sees an uninitialised index
__global__ void sqnorm_kernel(const float* __restrict__ x, int ld, int P, int C, float* __restrict__ xx, int* __restrict__ idx, int k) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    if (idx)
        for (int s = 0; s < k; ++s) idx[(size_t)i * k + s] = 0;
    const float* r = x + (size_t)i * ld;
    float acc = 0.f;
    if ((C & 3) == 0 && (ld & 3) == 0 && (((uintptr_t)x) & 15) == 0) {      // same chain (c ascending), 16-byte loads, four in flight
        int c = 0;
        for (; c + 16 <= C; c += 16) {
            const f32x4 a = *(const f32x4*)(r + c), b = *(const f32x4*)(r + c + 4), d = *(const f32x4*)(r + c + 8), e = *(const f32x4*)(r + c + 12);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fmaf(a[u], a[u], acc);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fmaf(b[u], b[u], acc);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fmaf(d[u], d[u], acc);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fmaf(e[u], e[u], acc);
        }
        for (; c < C; c += 4) {
            const f32x4 a = *(const f32x4*)(r + c);
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fmaf(a[u], a[u], acc);
        }
    } else {
        for (int c = 0; c < C; ++c) acc = fmaf(r[c], r[c], acc);
    }
    xx[i] = acc;
}

template <int KMAX>
struct TopK {
    float v[KMAX];
    int id[KMAX];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int s = 0; s < KMAX; ++s) { v[s] = -INFINITY; id[s] = 0x7fffffff; }
    }
    // candidate beats entry (pv,pi)?  total order: value desc, index asc
    static __device__ __forceinline__ bool beats(float d, int j, float pv, int pi) {
        return d > pv || (d == pv && j < pi);
    }
    __device__ __forceinline__ void insert(float d, int j) {
#pragma unroll
        for (int s = KMAX - 1; s >= 1; --s) {
            bool up = beats(d, j, v[s - 1], id[s - 1]);
            bool here = beats(d, j, v[s], id[s]);
            float nv = up ? v[s - 1] : (here ? d : v[s]);
            int ni = up ? id[s - 1] : (here ? j : id[s]);
            v[s] = nv; id[s] = ni;
        }
        bool first = beats(d, j, v[0], id[0]);
        v[0] = first ? d : v[0];
        id[0] = first ? j : id[0];
    }
};

// CT > 0: compile-time channel count (query in registers).  CT == 0: runtime C (query in LDS).
template <int KMAX, int CT>
__global__ __launch_bounds__(256) void knn_kernel(const float* __restrict__ x, const float* __restrict__ xx_all,
                                                  int ld, int N, int C, int k, int* __restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int q = blockIdx.x * KNN_QB + lane;          // query (local index in its cloud)
    const bool qvalid = q < N;
    const float* xb = x + (size_t)b * N * ld;
    const float* xxb = xx_all + (size_t)b * N;
    const int Cr = CT > 0 ? CT : C;

    // LDS carve: [4 waves][TJ][Cr] candidate tiles | [4][TJ] candidate norms | (CT==0) [64][Cr+1] queries
    float* cand = sm + (size_t)wave * KNN_TJ * Cr;
    float* cxx = sm + (size_t)4 * KNN_TJ * Cr + wave * KNN_TJ;
    float* qs = sm + (size_t)4 * KNN_TJ * Cr + 4 * KNN_TJ;

    float qreg[CT > 0 ? CT : 1];
    if (CT > 0) {
#pragma unroll
        for (int c = 0; c < (CT > 0 ? CT : 1); ++c) qreg[c] = qvalid ? xb[(size_t)q * ld + c] : 0.f;
    } else {
        for (int e = tid; e < KNN_QB * Cr; e += 256) {
            int qq = e / Cr, c = e % Cr;
            int gq = blockIdx.x * KNN_QB + qq;
            qs[qq * (Cr + 1) + c] = gq < N ? xb[(size_t)gq * ld + c] : 0.f;
        }
        __syncthreads();
    }
    const float xxi = qvalid ? xxb[q] : 0.f;

    TopK<KMAX> top;
    top.init();

    // this wave's candidate range
    const int per = (N + 3) / 4;
    const int jbeg = wave * per, jend = min(N, jbeg + per);
    for (int j0 = jbeg; j0 < jend; j0 += KNN_TJ) {
        const int nj = min(KNN_TJ, jend - j0);
        // stage tile (wave-private region: no workgroup barrier needed, only wave-level ordering)
        for (int e = lane; e < nj * Cr; e += 64) cand[e] = xb[(size_t)(j0 + e / Cr) * ld + (e % Cr)];
        if (lane < nj) cxx[lane] = xxb[j0 + lane];
        __builtin_amdgcn_s_waitcnt(0);   // vmcnt(0) lgkmcnt(0): LDS writes of this wave are done
        __builtin_amdgcn_wave_barrier();
        for (int jj = 0; jj < nj; ++jj) {
            const float* cj = cand + jj * Cr;
            float dot = 0.f;
            if (CT > 0) {
#pragma unroll
                for (int c = 0; c < (CT > 0 ? CT : 1); ++c) dot = fmaf(qreg[c], cj[c], dot);
            } else {
                const float* qr = qs + lane * (Cr + 1);
                for (int c = 0; c < Cr; ++c) dot = fmaf(qr[c], cj[c], dot);
            }
            float t = fmaf(2.0f, dot, -cxx[jj]);
            float pd = t - xxi;
            // ascending j inside a wave: a later equal value never displaces an earlier one
            if (__any(pd > top.v[KMAX - 1])) top.insert(pd, j0 + jj);
        }
        __builtin_amdgcn_wave_barrier();
    }

    // merge the 4 partial lists: waves 1..3 publish theirs, wave 0 inserts them
    __syncthreads();                         // everyone is done with the candidate tiles
    float* mv = sm;                          // [3][KMAX][64] values
    int* mi = (int*)(sm + 3 * KMAX * 64);    // [3][KMAX][64] indices
    if (wave > 0) {
#pragma unroll
        for (int s = 0; s < KMAX; ++s) {
            mv[((wave - 1) * KMAX + s) * 64 + lane] = top.v[s];
            mi[((wave - 1) * KMAX + s) * 64 + lane] = top.id[s];
        }
    }
    __syncthreads();
    if (wave == 0) {
        for (int w = 0; w < 3; ++w)
            for (int s = 0; s < KMAX; ++s) {
                float d = mv[(w * KMAX + s) * 64 + lane];
                int j = mi[(w * KMAX + s) * 64 + lane];
                if (__any(TopK<KMAX>::beats(d, j, top.v[KMAX - 1], top.id[KMAX - 1]))) top.insert(d, j);
            }
        if (qvalid) {
            int* o = idx + ((size_t)b * N + q) * k;
#pragma unroll
            for (int s = 0; s < KMAX; ++s)
                if (s < k) o[s] = top.id[s];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Distance tiles on the matrix cores (every kernel below).  D[cand 32][query 32] = Xc Xq^T by v_mfma_f32_32x32x2_f32, which is
// bit-for-bit a k-ordered fmaf chain (c = 2s on lanes 0-31, c = 2s+1 on lanes 32-63), i.e. exactly the canonical dot product.
// Candidate tiles are staged k-major through LDS [c][33]; channels are zero-padded to CT (fmaf(0,0,acc) == acc, so padding does not
// perturb the chain).  (The round-1 list-merge kernel that kept k sorted entries per lane -- and spilled for k = 40 -- is gone: its
// shapes run on the two-pass kernel, the few it does not take on the VALU kernel above.)
#define KM_STRIDE 33

template <int CT>
__global__ __launch_bounds__(256) void knn_mfma3_kernel(const float* __restrict__ x, const float* __restrict__ xx_all,
                                                        int ld, int N, int C, int k, int vec_ok, int* __restrict__ idx) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int TILE = CT * KM_STRIDE;
    constexpr int NSTEP = CT / 2;
    constexpr int SPR = NSTEP >= 16 ? NSTEP / 16 : 1;       // MFMA steps issued per query row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int b = blockIdx.y;
    const float* xb = x + (size_t)b * N * ld;
    const float* xxb = xx_all + (size_t)b * N;
    float* tiles = sm;                                    // [2][CT][33]
    float* cxx = sm + 2 * TILE;                           // [3][32]  (norms of tiles t, t+1, t+2 are live at once)

    const int q0 = blockIdx.x * 128 + wave * 32;          // first query of this wave
    float qa[NSTEP];
    {
        const int q = q0 + l31;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            int c = 2 * s + h;
            qa[s] = (q < N && c < C) ? xb[(size_t)q * ld + c] : 0.f;
        }
    }
    float xxq[16], lv[16], thr[16];
    int li[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int q = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        xxq[r] = q < N ? xxb[q] : 0.f;
        lv[r] = -INFINITY; thr[r] = -INFINITY; li[r] = 0x7fffffff;
    }

    const int ntiles = (N + 31) / 32;
    constexpr int NLD = (32 * CT / 4 + 255) / 256;
    f32x4 stage[NLD];
    auto g2r_tile = [&](int t) {
        const int j0 = t * 32;
#pragma unroll
        for (int p = 0; p < NLD; ++p) {
            int f = tid + 256 * p;
            int cand = f / (CT / 4), c = (f % (CT / 4)) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (f < 32 * CT / 4 && t < ntiles && j0 + cand < N) {
                const float* g = xb + (size_t)(j0 + cand) * ld + c;
                if (vec_ok && c + 3 < C) v = *(const f32x4*)g;
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (c + e < C) v[e] = g[e];
                }
            }
            stage[p] = v;
        }
    };
    auto r2s_tile = [&](int buf, int t) {
        float* T = tiles + buf * TILE;
#pragma unroll
        for (int p = 0; p < NLD; ++p) {
            int f = tid + 256 * p;
            if (f < 32 * CT / 4) {
                int cand = f / (CT / 4), c = (f % (CT / 4)) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) T[(c + e) * KM_STRIDE + cand] = stage[p][e];
            }
        }
        if (tid < 32) {
            int j = t * 32 + tid;
            cxx[(t % 3) * 32 + tid] = (t < ntiles && j < N) ? xxb[j] : 0.f;
        }
    };

    f32x16 accCur, accNext;
#pragma unroll
    for (int r = 0; r < 16; ++r) { accCur[r] = 0.f; accNext[r] = 0.f; }
    // prologue: tile 0 -> buf 0, compute it; tile 1 -> buf 1
    g2r_tile(0);
    r2s_tile(0, 0);
    __syncthreads();
    {
        const float* T = tiles + h * KM_STRIDE + l31;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s)
            accCur = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[s], T[(2 * s) * KM_STRIDE], accCur, 0, 0, 0);
    }
    g2r_tile(1);
    r2s_tile(1, 1);

    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                       // tile t+1 visible in buf (t+1)&1; buf t&1 free for tile t+2
        const bool have_next = t + 1 < ntiles;
        if (t + 2 < ntiles) g2r_tile(t + 2);
        const float* T = tiles + ((t + 1) & 1) * TILE + h * KM_STRIDE + l31;
        const float xxc = cxx[(t % 3) * 32 + l31];
        const int j = t * 32 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) accNext[r] = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            // slice of the next tile's MFMA chain
            if (have_next && r * SPR < NSTEP) {
#pragma unroll
                for (int u = 0; u < SPR; ++u) {
                    const int s = r * SPR + u;
                    accNext = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[s], T[(2 * s) * KM_STRIDE], accNext, 0, 0, 0);
                }
            }
            // selection for query row r of the current tile
            float pd = fmaf(2.0f, accCur[r], -xxc) - xxq[r];
            if (j >= N) pd = -INFINITY;
            unsigned long long m = __ballot(pd > thr[r]);
            if (m) {
                // everything that steers the insertion is wave-uniform (the ballot is an SGPR pair): the survivor of
                // each half is broadcast with v_readlane, the tail shifts down one lane with a DPP wave_shr -- no
                // LDS-routed shuffles on this path
                unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
                const int pdi = __float_as_int(pd);
                while (lo | hi) {
                    const int s0 = lo ? __builtin_ctz(lo) : 0, s1 = hi ? __builtin_ctz(hi) : 0;
                    const float x0 = __int_as_float(__builtin_amdgcn_readlane(pdi, s0));
                    const float x1 = __int_as_float(__builtin_amdgcn_readlane(pdi, 32 + s1));
                    const bool active = h ? (hi != 0) : (lo != 0);
                    const float xv = h ? x1 : x0;
                    const int xj = t * 32 + (h ? s1 : s0);
                    const float upv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(lv[r]), 0x138, 0xf, 0xf, false));
                    const int upi = __builtin_amdgcn_update_dpp(0, li[r], 0x138, 0xf, 0xf, false);
                    const bool lt = lv[r] < xv;                       // ties keep the earlier (lower index) entry ahead
                    const bool uplt = (l31 > 0) && (upv < xv);
                    if (active && lt) { lv[r] = uplt ? upv : xv; li[r] = uplt ? upi : xj; }
                    lo &= lo - 1; hi &= hi - 1;
                }
                const float t0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lv[r]), k - 1));
                const float t1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lv[r]), 32 + k - 1));
                thr[r] = h ? t1 : t0;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (t + 2 < ntiles) r2s_tile(t & 1, t + 2);
#pragma unroll
        for (int r = 0; r < 16; ++r) accCur[r] = accNext[r];
    }

    // lane l31 < k of each half holds rank l31 of query row rho(r,h)
    if (l31 < k) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (q < N) idx[((size_t)b * N + q) * k + l31] = li[r];
        }
    }
}

template <int CT>
static int launch_knn_mfma3_ct(hipStream_t st, const float* x, int ld, const float* xx, int B, int N, int C, int k, int* idx) {
    size_t lds = ((size_t)2 * CT * KM_STRIDE + 96) * sizeof(float);
    if (lds > 160 * 1024) return MLSP_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        hipError_t e = mlsp_lds_limit((const void*)knn_mfma3_kernel<CT>, lds);
        if (e != hipSuccess) return (int)e;
    }
    int vec_ok = (ld % 4 == 0) && (((uintptr_t)x & 15) == 0);
    dim3 grid((N + 127) / 128, B);
    hipLaunchKernelGGL((knn_mfma3_kernel<CT>), grid, dim3(256), lds, st, x, xx, ld, N, C, k, vec_ok, idx);
    return mlsp_launch_status();
}

static int launch_knn_mfma3(hipStream_t st, const float* x, int ld, const float* xx, int B, int N, int C, int k, int* idx) {
    if (C <= 4) return launch_knn_mfma3_ct<4>(st, x, ld, xx, B, N, C, k, idx);
    if (C <= 16) return launch_knn_mfma3_ct<16>(st, x, ld, xx, B, N, C, k, idx);
    if (C <= 64) return launch_knn_mfma3_ct<64>(st, x, ld, xx, B, N, C, k, idx);
    if (C <= 128) return launch_knn_mfma3_ct<128>(st, x, ld, xx, B, N, C, k, idx);
    if (C <= 256) return launch_knn_mfma3_ct<256>(st, x, ld, xx, B, N, C, k, idx);
    return MLSP_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------
// v4: two-pass threshold select on top of the v3 tile pipeline (same canonical distances, same total order).
//   pass A  every lane keeps the running max of ITS column of the distance tiles (one v_max per value): 32 disjoint
//           chunk maxima per query.  The k-th largest of them, tau, is a lower bound of the k-th best distance (k
//           chunks each hold a value >= tau), so only candidates with pd >= tau can be in the answer (~30 of 1024).
//   pass B  recompute the tiles (the MFMA sweep is 20-60 us, the selection was 300); survivors are appended to a
//           per-query LDS buffer by ballot + prefix count -- no per-candidate loop.
//   final   exact rank of every survivor by counting (value desc, index asc): rank < k -> idx[q][rank].
// If any query of the workgroup overflows its 64-entry buffer (massive ties) the workgroup re-runs the v3
// sequential insertion (pass C), which is exact for any input.
#define KNN4_CAP 64

template <int CT>
__global__ __launch_bounds__(256) void knn_mfma4_kernel(const float* __restrict__ x, const float* __restrict__ xx_all,
                                                        int ld, int N, int C, int k, int vec_ok, int* __restrict__ idx, int B) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int TILE = CT * KM_STRIDE;
    constexpr int NSTEP = CT / 2;
    constexpr int SPR = NSTEP >= 16 ? NSTEP / 16 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    int b, chunk;
    xcd_cloud_map(blockIdx.x, (N + 127) / 128, B, b, chunk);
    const float* xb = x + (size_t)b * N * ld;
    const float* xxb = xx_all + (size_t)b * N;
    float* tiles = sm;                                    // [2][CT][33]
    float* cxx = sm + 2 * TILE;                           // [3][32]
    float* bufv = cxx + 96 + wave * 32 * KNN4_CAP;        // [32 queries][CAP] survivor values of this wave
    int* bufj = (int*)(cxx + 96 + 4 * 32 * KNN4_CAP) + wave * 32 * KNN4_CAP;

    const int q0 = chunk * 128 + wave * 32;
    float qa[NSTEP];
    {
        const int q = q0 + l31;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            int c = 2 * s + h;
            qa[s] = (q < N && c < C) ? xb[(size_t)q * ld + c] : 0.f;
        }
    }
    float xxq[16], thr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int q = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        xxq[r] = q < N ? xxb[q] : 0.f;
        thr[r] = -INFINITY;
    }

    const int ntiles = (N + 31) / 32;
    constexpr int NLD = (32 * CT / 4 + 255) / 256;
    f32x4 stage[NLD];
    float xxstage = 0.f;                                  // candidate norms travel with the tile (no exposed load in r2s)
    auto g2r_tile = [&](int t) {
        const int j0 = t * 32;
        if (tid < 32) xxstage = (t < ntiles && j0 + tid < N) ? xxb[j0 + tid] : 0.f;
#pragma unroll
        for (int p = 0; p < NLD; ++p) {
            int f = tid + 256 * p;
            int cand = f / (CT / 4), c = (f % (CT / 4)) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (f < 32 * CT / 4 && t < ntiles && j0 + cand < N) {
                const float* g = xb + (size_t)(j0 + cand) * ld + c;
                if (vec_ok && c + 3 < C) v = *(const f32x4*)g;
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) if (c + e < C) v[e] = g[e];
                }
            }
            stage[p] = v;
        }
    };
    auto r2s_tile = [&](int buf, int t) {
        float* T = tiles + buf * TILE;
#pragma unroll
        for (int p = 0; p < NLD; ++p) {
            int f = tid + 256 * p;
            if (f < 32 * CT / 4) {
                int cand = f / (CT / 4), c = (f % (CT / 4)) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) T[(c + e) * KM_STRIDE + cand] = stage[p][e];
            }
        }
        if (tid < 32) cxx[(t % 3) * 32 + tid] = xxstage;
    };

    // one full sweep over the candidate tiles; sel(r, pd, t) is invoked for every query row of every tile
    auto sweep = [&](auto&& sel) {
        f32x16 accCur, accNext;
#pragma unroll
        for (int r = 0; r < 16; ++r) { accCur[r] = 0.f; accNext[r] = 0.f; }
        __syncthreads();                       // previous sweep is done with the tile buffers
        g2r_tile(0);
        r2s_tile(0, 0);
        __syncthreads();
        {
            const float* T = tiles + h * KM_STRIDE + l31;
#pragma unroll
            for (int s = 0; s < NSTEP; ++s)
                accCur = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[s], T[(2 * s) * KM_STRIDE], accCur, 0, 0, 0);
        }
        g2r_tile(1);
        r2s_tile(1, 1);
        for (int t = 0; t < ntiles; ++t) {
            __syncthreads();
            const bool have_next = t + 1 < ntiles;
            if (t + 2 < ntiles) g2r_tile(t + 2);
            const float* T = tiles + ((t + 1) & 1) * TILE + h * KM_STRIDE + l31;
            const float xxc = cxx[(t % 3) * 32 + l31];
            const int j = t * 32 + l31;
            // all B fragments of the next tile are fetched up front: the MFMA slices below then never wait on LDS
            float bf[NSTEP];
#pragma unroll
            for (int s = 0; s < NSTEP; ++s) bf[s] = T[(2 * s) * KM_STRIDE];
#pragma unroll
            for (int r = 0; r < 16; ++r) accNext[r] = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (have_next && r * SPR < NSTEP) {
#pragma unroll
                    for (int u = 0; u < SPR; ++u) {
                        const int s = r * SPR + u;
                        accNext = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[s], bf[s], accNext, 0, 0, 0);
                    }
                }
                float pd = fmaf(2.0f, accCur[r], -xxc) - xxq[r];
                if (j >= N) pd = -INFINITY;
                sel(r, pd, t);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (t + 2 < ntiles) r2s_tile(t & 1, t + 2);
#pragma unroll
            for (int r = 0; r < 16; ++r) accCur[r] = accNext[r];
        }
    };

    // ---- pass A: per-lane chunk maxima -> tau = k-th largest of the 32 lane values of each query
    float cm[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) cm[r] = -INFINITY;
    sweep([&](int r, float pd, int) { cm[r] = fmaxf(cm[r], pd); });
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ci = __float_as_int(cm[r]);
        int rank = 0;
        for (int i = 0; i < 32; ++i) {
            const float x0 = __int_as_float(__builtin_amdgcn_readlane(ci, i));
            const float x1 = __int_as_float(__builtin_amdgcn_readlane(ci, 32 + i));
            const float xv = h ? x1 : x0;
            rank += (xv > cm[r] || (xv == cm[r] && i < l31)) ? 1 : 0;
        }
        const unsigned long long m = __ballot(rank == k - 1);
        const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
        const float t0 = __int_as_float(__builtin_amdgcn_readlane(ci, lo ? __builtin_ctz(lo) : 0));
        const float t1 = __int_as_float(__builtin_amdgcn_readlane(ci, 32 + (hi ? __builtin_ctz(hi) : 0)));
        thr[r] = h ? t1 : t0;
    }

    // ---- pass B: ballot-compaction of the survivors (pd >= tau) into the per-query buffers
    int cnt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) cnt[r] = 0;
    sweep([&](int r, float pd, int t) {
        const bool pass = pd >= thr[r];
        const unsigned long long m = __ballot(pass);
        if (m) {
            const unsigned mine = h ? (unsigned)(m >> 32) : (unsigned)m;
            const int pos = cnt[r] + __builtin_popcount(mine & ((1u << l31) - 1u));
            if (pass && pos < KNN4_CAP) {
                const int qrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                bufv[qrow * KNN4_CAP + pos] = pd;
                bufj[qrow * KNN4_CAP + pos] = t * 32 + l31;
            }
            cnt[r] += __builtin_popcount(mine);
        }
    });
    bool over = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) over |= cnt[r] > KNN4_CAP;

    if (!__syncthreads_or(over ? 1 : 0)) {
        // ---- exact rank select among the survivors
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qrow = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int q = q0 + qrow;
            const int n = cnt[r];
            const float* bv = bufv + qrow * KNN4_CAP;
            const int* bj = bufj + qrow * KNN4_CAP;
            const float v0 = l31 < n ? bv[l31] : -INFINITY, v1 = l31 + 32 < n ? bv[l31 + 32] : -INFINITY;
            const int j0 = l31 < n ? bj[l31] : 0x7fffffff, j1 = l31 + 32 < n ? bj[l31 + 32] : 0x7fffffff;
            const int nmax = max(__builtin_amdgcn_readlane(n, 0), __builtin_amdgcn_readlane(n, 32));
            int rank0 = 0, rank1 = 0;
            for (int i = 0; i < nmax; ++i) {
                const float xv = i < n ? bv[i] : -INFINITY;
                const int xj = i < n ? bj[i] : 0x7fffffff;
                rank0 += (xv > v0 || (xv == v0 && xj < j0)) ? 1 : 0;
                rank1 += (xv > v1 || (xv == v1 && xj < j1)) ? 1 : 0;
            }
            if (q < N) {
                if (l31 < n && rank0 < k) idx[((size_t)b * N + q) * k + rank0] = j0;
                if (l31 + 32 < n && rank1 < k) idx[((size_t)b * N + q) * k + rank1] = j1;
            }
        }
        return;
    }

    // ---- pass C (fallback, exact for any input): v3 sequential insertion into lane-distributed sorted lists
    float lv[16];
    int li[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { lv[r] = -INFINITY; li[r] = 0x7fffffff; thr[r] = -INFINITY; }
    sweep([&](int r, float pd, int t) {
        unsigned long long m = __ballot(pd > thr[r]);
        if (m) {
            unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
            const int pdi = __float_as_int(pd);
            while (lo | hi) {
                const int s0 = lo ? __builtin_ctz(lo) : 0, s1 = hi ? __builtin_ctz(hi) : 0;
                const float x0 = __int_as_float(__builtin_amdgcn_readlane(pdi, s0));
                const float x1 = __int_as_float(__builtin_amdgcn_readlane(pdi, 32 + s1));
                const bool active = h ? (hi != 0) : (lo != 0);
                const float xv = h ? x1 : x0;
                const int xj = t * 32 + (h ? s1 : s0);
                const float upv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(lv[r]), 0x138, 0xf, 0xf, false));
                const int upi = __builtin_amdgcn_update_dpp(0, li[r], 0x138, 0xf, 0xf, false);
                const bool lt = lv[r] < xv;
                const bool uplt = (l31 > 0) && (upv < xv);
                if (active && lt) { lv[r] = uplt ? upv : xv; li[r] = uplt ? upi : xj; }
                lo &= lo - 1; hi &= hi - 1;
            }
            const float t0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lv[r]), k - 1));
            const float t1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lv[r]), 32 + k - 1));
            thr[r] = h ? t1 : t0;
        }
    });
    if (l31 < k) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (q < N) idx[((size_t)b * N + q) * k + l31] = li[r];
        }
    }
}

template <int CT>
static int launch_knn_mfma4_ct(hipStream_t st, const float* x, int ld, const float* xx, int B, int N, int C, int k, int* idx) {
    size_t lds = ((size_t)2 * CT * KM_STRIDE + 96 + 2 * 4 * 32 * KNN4_CAP) * sizeof(float);
    if (lds > 160 * 1024) return MLSP_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        hipError_t e = mlsp_lds_limit((const void*)knn_mfma4_kernel<CT>, lds);
        if (e != hipSuccess) return (int)e;
    }
    int vec_ok = (ld % 4 == 0) && (((uintptr_t)x & 15) == 0);
    dim3 grid(((N + 127) / 128) * B);
    hipLaunchKernelGGL((knn_mfma4_kernel<CT>), grid, dim3(256), lds, st, x, xx, ld, N, C, k, vec_ok, idx, B);
    return mlsp_launch_status();
}

static int launch_knn_mfma4(hipStream_t st, const float* x, int ld, const float* xx, int B, int N, int C, int k, int* idx) {
    if (C <= 4) return launch_knn_mfma4_ct<4>(st, x, ld, xx, B, N, C, k, idx);
    if (C <= 16) return launch_knn_mfma4_ct<16>(st, x, ld, xx, B, N, C, k, idx);
    if (C <= 64) return launch_knn_mfma4_ct<64>(st, x, ld, xx, B, N, C, k, idx);
    if (C <= 128) return launch_knn_mfma4_ct<128>(st, x, ld, xx, B, N, C, k, idx);
    return MLSP_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------
// v5: the v4 two-pass threshold select with the candidates of a query split over TWO waves.
// A workgroup is 8 waves = 4 query groups (32 queries each) x 2 candidate halves, so every SIMD holds two waves and one
// wave's LDS / barrier / selection latency is covered by the other's MFMA work (v4 ran one wave per SIMD: its sweeps took
// 2x the MFMA-bound time).  Same canonical distances and the same total order (pd desc, index asc) as v1-v4:
//   pass A  per-lane running maxima over the wave's half: 2 x 32 chunk maxima per query, exchanged through LDS;
//           tau = k-th largest of the 64 (a lower bound of the k-th best distance, ~24 survivors of 1024 expected).
//   pass B  survivors (pd >= tau) of each half are appended, as 64-bit sortable keys, to that wave's 32-entry buffer.
//   final   rank of every key among the <= 64 keys of the query by counting; rank < k -> idx[q][rank].
//   pass C  (any buffer overflowed: massive ties) each wave runs the v3 sequential insertion over its half and
//           publishes its exact top-k as keys; the same final merges the two halves.
// RES (CT <= 16): the whole cloud's candidates stay in LDS for both passes, no per-tile barriers.
// Requires N % 128 == 0 (full query chunks, an even number of 32-candidate tiles); everything else stays on v4.
//
// KB = 1 (24 < k <= 64; BASELINE.json configs[4] asks k = 40): the same two passes with a finer bound and a shared buffer:
//   pass A  TWO running maxima per lane (first / second half of the wave's tiles): 128 chunk maxima per query; tau = k-th
//           largest of the 128 = two 64-sorts (both halves of a wave: lane l sorts the maxima of candidate half 0, lane l+32
//           those of half 1), one cross-half max layer (top 64 of the union, bitonic) and a 6-stage bitonic merge.
//           k = 40 of 128 maxima leaves ~47 +- 7 survivors of 2048 candidates.
//   pass B  survivors of BOTH halves go to ONE buffer of KNN5_CAPT keys per query (LDS atomic on the query's counter per
//           ballot hit -- hits are rare, ~47 per query over the whole sweep), so the capacity covers the SUM of the halves.
//   pass C  (overflow: massive ties) lane-distributed sorted lists with two entries per lane (positions l and 32 + l);
//           the halves publish one after the other through the same buffer and rank their own keys against the other's.
// The query fragments are re-read from global memory after the tau phase instead of staying live across it (registers).
#define KNN5_CAP 32
#define KNN5_CAPT 88               // KB = 1: keys per query, both halves together (16-byte aligned rows)
#define KNN5_XS 68                 // row stride (floats) of the pass-A exchange image: 16 B aligned rows, 2-way banked
typedef unsigned long long u64;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u64 knn_key(float pd, int j) {
    pd += 0.0f;                                            // -0 -> +0: keys order exactly like the float compare
    unsigned u = (unsigned)__float_as_int(pd);
    u ^= (unsigned)((int)u >> 31) | 0x80000000u;           // monotone float -> unsigned
    return ((u64)u << 32) | (unsigned)(~j);                // larger key = (larger pd, then smaller index)
}

// ---- pass A on the bf16 matrix cores (streaming variants, C = 64 and C = 128 with k <= 24) ------------------------------------------------
// Pass A only has to produce a LOWER BOUND tau of a query's k-th best distance; pass B (exact fp32, canonical arithmetic) decides the
// result.  So pass A may use approximate distances: x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (|x - hi - lo| <= 2^-17 |x|),
//   dot' = sum hi_q hi_j + hi_q lo_j + lo_q hi_j      (3 x C/16 v_mfma_f32_32x32x16_bf16 per 32x32 tile instead of C/2 fp32 MFMAs)
// |2 dot' - 2 dot| <= 2^-15 |x_q| |x_j| (dropped lo lo term, the two residuals) + fp32 accumulation (C 2^-24), so with the final
// roundings  |pd' - pd| < 2^-15.3 (xx_q + max_j xx_j).  tau' = k-th largest of the approximate chunk maxima; at least k candidates have
// pd' >= tau', hence pd >= tau' - eps: tau = tau' - eps_q with eps_q = 2^-14 (xx_q + max_j xx_j) is still a proven bound (a NaN bound
// becomes -inf: everything survives, the exact fallback sweep takes over).  A few more survivors reach pass B; the indices stay bit-exact.
typedef __bf16 kbf16x8 __attribute__((ext_vector_type(8)));
#define KNN5_EPS 1.220703125e-04f           // 2^-13: worst-case budget of the split products + fp32 accumulation is 2^-13.9 (knn6.hip header)
__device__ __forceinline__ void knn_split8(const float (&b)[8], kbf16x8& hi, kbf16x8& lo) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const __bf16 hv = (__bf16)b[e];
        hi[e] = hv;
        lo[e] = (__bf16)(b[e] - (float)hv);
    }
}

template <int CT, bool VEC, bool RES, int KB>
__global__ __launch_bounds__(512) void knn_mfma5_kernel(const float* __restrict__ x, const float* __restrict__ xx_all,
                                                        int ld, int N, int C, int k, int* __restrict__ idx, int B, const int* __restrict__ only_clouds) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int TILE = CT * KM_STRIDE;
    constexpr bool AP = (CT == 64 || (CT == 128 && KB == 0)) && !RES && VEC;     // pass A on the bf16 matrix cores (header comment above the kernel; C = 128 with k > 24 is out of registers)
    constexpr int PA = CT + 8;                              // bf16 elements per candidate row of a pass-A image (16-byte aligned rows)
    constexpr int TILEA = 32 * PA;                          // floats of one pass-A tile image: hi rows [32][PA] bf16, then lo rows
    constexpr int TILE_ALLOC = (AP && TILEA > TILE) ? TILEA : TILE;
    constexpr int NSTEP = CT / 2;
    constexpr int SPR = NSTEP >= 16 ? NSTEP / 16 : 1;      // MFMA steps issued per query row of the select loop
    constexpr int GS = (KB && CT == 128) ? 4 : NSTEP >= 16 ? 16 : NSTEP;   // B fragments fetched per group (the k > 24 variant at C = 128 is out of registers)
    constexpr int NG = NSTEP / GS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int qg = wave & 3, ch = wave >> 2, ht = tid & 255;
    int b, chunk;
    xcd_cloud_map(blockIdx.x, N / 128, B, b, chunk);
    if (only_clouds && only_clouds[b] == 0) return;             // behind knn6w_kernel: only the clouds it flagged (uniform per workgroup)
    const float* xb = x + (size_t)b * N * ld;
    const float* xxb = xx_all + (size_t)b * N;
    const int ntiles = N / 32, nt2 = ntiles / 2;

    float* tiles = sm;                                           // RES: [ntiles][CT][33]   else [2 halves][2][CT][33]
    float* cxx = tiles + (RES ? (size_t)ntiles * TILE : (size_t)4 * TILE_ALLOC);   // RES: [N]   else [2 halves][3][32]
    u64* bufk = (u64*)(cxx + (RES ? N : 192));                   // KB=0: [4 qg][2 ch][32 queries][CAP] survivor keys; KB=1: [128 queries][CAPT]
    float* xch = (float*)bufk;                                   // pass-A exchange [4][2][(2 parts)][16][XS], dead before pass B
    float* tau = (float*)(bufk + (KB ? 128 * KNN5_CAPT : 4 * 2 * 32 * KNN5_CAP));   // [4 qg][16 rows][2 h]
    int* cnts = (int*)(tau + 128);                               // KB=0: [4 qg][2 ch][32 queries]; KB=1: [4 qg][32 queries]

    const int q0 = chunk * 128 + qg * 32;
    float qa[NSTEP];
    auto load_queries = [&]() {
        const int q = q0 + l31;
#pragma unroll
        for (int s = 0; s < NSTEP; ++s) {
            int c = 2 * s + h;
            qa[s] = (c < C) ? xb[(size_t)q * ld + c] : 0.f;
        }
    };
    constexpr int NKB = CT / 16;
    kbf16x8 qhi[AP ? NKB : 1], qlo[AP ? NKB : 1];          // the query row's hi / lo halves, channels 16 kb + 8 h .. + 7
    float xxmax = 0.f;
    if (AP) {
        const int q = q0 + l31;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            float t[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { const int c = 16 * kb + 8 * h + e; t[e] = c < C ? xb[(size_t)q * ld + c] : 0.f; }
            knn_split8(t, qhi[kb], qlo[kb]);
        }
        // largest squared norm of the cloud (the error bound of a distance scales with xx_q + xx_j)
        __shared__ float xxm_s[8];
        float m = 0.f;
        for (int j = tid; j < N; j += 512) m = fmaxf(m, xxb[j]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (lane == 0) xxm_s[wave] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 8; ++w) xxmax = fmaxf(xxmax, xxm_s[w]);
    } else {
        load_queries();
    }
    float xxq[16], thr[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        xxq[r] = xxb[q0 + (r & 3) + 8 * (r >> 2) + 4 * h];
        thr[r] = -INFINITY;
    }

    if (RES) {
        // the whole cloud, once: tile t at tiles + t*TILE, k-major [c][33]
        if (VEC) {
            for (int f = tid; f < N * (CT / 4); f += 512) {
                const int cand = f / (CT / 4), c = (f % (CT / 4)) * 4;
                const f32x4 v = *(const f32x4*)(xb + (size_t)cand * ld + c);
                float* T = tiles + (cand >> 5) * TILE + (cand & 31);
#pragma unroll
                for (int e = 0; e < 4; ++e) T[(c + e) * KM_STRIDE] = v[e];
            }
        } else {
            for (int f = tid; f < N * CT; f += 512) {
                const int cand = f / CT, c = f % CT;
                tiles[(cand >> 5) * TILE + c * KM_STRIDE + (cand & 31)] = c < C ? xb[(size_t)cand * ld + c] : 0.f;
            }
        }
        for (int j = tid; j < N; j += 512) cxx[j] = xxb[j];
    }

    // streaming mode: the 256 threads of a half stage that half's tiles (registers -> LDS, k-major)
    constexpr int NLD = VEC ? (32 * CT / 4 + 255) / 256 : (32 * CT + 255) / 256;
    f32x4 stagev[VEC ? NLD : 1];
    float stages[VEC ? 1 : NLD];
    float xxstage = 0.f;
    float* htiles = tiles + ch * 2 * TILE_ALLOC;
    float* hcxx = cxx + ch * 96;
    auto g2r_tile = [&](int tl) {                          // tl: tile index inside the half, < nt2
        const int j0 = (ch * nt2 + tl) * 32;
        if (ht < 32) xxstage = xxb[j0 + ht];
        if (VEC) {
#pragma unroll
            for (int p = 0; p < NLD; ++p) {
                const int f = ht + 256 * p;
                if (32 * CT / 4 >= 256 * (p + 1) || f < 32 * CT / 4)
                    stagev[p] = *(const f32x4*)(xb + (size_t)(j0 + f / (CT / 4)) * ld + (f % (CT / 4)) * 4);
            }
        } else {
#pragma unroll
            for (int p = 0; p < NLD; ++p) {
                const int f = ht + 256 * p;
                const int cand = f / CT, c = f % CT;
                stages[p] = (f < 32 * CT && c < C) ? xb[(size_t)(j0 + cand) * ld + c] : 0.f;
            }
        }
    };
    // pass-A image of a tile: every candidate row split into bf16 hi / lo ONCE, by the thread that staged it (the four query-group
    // waves of the half then read ready-made 16-byte fragments)
    auto r2s_tileA = [&](int buf, int tl) {
        __bf16* Ih = (__bf16*)(htiles + buf * TILE_ALLOC);
        __bf16* Il = Ih + 32 * PA;
#pragma unroll
        for (int p = 0; p < NLD; ++p) {
            const int f = ht + 256 * p;
            if (32 * CT / 4 >= 256 * (p + 1) || f < 32 * CT / 4) {
                const int cand = f / (CT / 4), c = (f % (CT / 4)) * 4;
                typedef __bf16 kbf16x4 __attribute__((ext_vector_type(4)));
                kbf16x4 hv, lv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = VEC ? stagev[p][e] : 0.f;
                    const __bf16 hh = (__bf16)v;
                    hv[e] = hh; lv[e] = (__bf16)(v - (float)hh);
                }
                *(kbf16x4*)(Ih + cand * PA + c) = hv;
                *(kbf16x4*)(Il + cand * PA + c) = lv;
            }
        }
        if (ht < 32) hcxx[(tl % 3) * 32 + ht] = xxstage;
    };
    auto r2s_tile = [&](int buf, int tl) {
        float* T = htiles + buf * TILE_ALLOC;
        if (VEC) {
#pragma unroll
            for (int p = 0; p < NLD; ++p) {
                const int f = ht + 256 * p;
                if (32 * CT / 4 >= 256 * (p + 1) || f < 32 * CT / 4) {
                    const int cand = f / (CT / 4), c = (f % (CT / 4)) * 4;
#pragma unroll
                    for (int e = 0; e < 4; ++e) T[(c + e) * KM_STRIDE + cand] = stagev[p][e];
                }
            }
        } else {
#pragma unroll
            for (int p = 0; p < NLD; ++p) {
                const int f = ht + 256 * p;
                if (f < 32 * CT) T[(f % CT) * KM_STRIDE + f / CT] = stages[p];
            }
        }
        if (ht < 32) hcxx[(tl % 3) * 32 + ht] = xxstage;
    };
    auto tile_ptr = [&](int tl) -> const float* {          // B-fragment base of tile tl of this wave's half
        return (RES ? tiles + (size_t)(ch * nt2 + tl) * TILE : htiles + (tl & 1) * TILE_ALLOC) + h * KM_STRIDE + l31;
    };

    // one sweep over the wave's half; sel(r, pd, j) sees every (query row, candidate) distance once; at_mid() runs between
    // the first and the second half of the wave's tiles (KB = 1 pass A snapshots its running maxima there)
    auto sweep = [&](auto&& sel, auto&& at_mid, auto approx_tag) {
        constexpr bool APX = AP && decltype(approx_tag)::value;        // this sweep computes its tiles with the split-bf16 products
        f32x16 accCur, accNext;
#pragma unroll
        for (int r = 0; r < 16; ++r) { accCur[r] = 0.f; accNext[r] = 0.f; }
        __syncthreads();                       // previous sweep is done with the tile buffers / RES image is complete
        // fragment of block kb of the pass-A image in buffer `buf`: candidate row l31, channels 16 kb + 8 h .. + 7 (one 16-byte read each)
        auto fragA = [&](int buf, int kb, kbf16x8& bh, kbf16x8& bl) {
            const __bf16* Ih = (const __bf16*)(htiles + buf * TILE_ALLOC) + l31 * PA + 16 * kb + 8 * h;
            bh = *(const kbf16x8*)Ih;
            bl = *(const kbf16x8*)(Ih + 32 * PA);
        };
        if (!RES) {
            g2r_tile(0);
            if (APX) r2s_tileA(0, 0); else r2s_tile(0, 0);
            __syncthreads();
        }
        if (APX) {
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                kbf16x8 bh, bl;
                fragA(0, kb, bh, bl);
                accCur = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qhi[kb], bh, accCur, 0, 0, 0);
                accCur = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qhi[kb], bl, accCur, 0, 0, 0);
                accCur = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qlo[kb], bh, accCur, 0, 0, 0);
            }
        } else {
            const float* T = tile_ptr(0);
#pragma unroll
            for (int s = 0; s < NSTEP; ++s)
                accCur = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[s], T[(2 * s) * KM_STRIDE], accCur, 0, 0, 0);
        }
        if (!RES) {
            g2r_tile(1);                       // nt2 >= 2 (N >= 128)
            if (APX) r2s_tileA(1, 1); else r2s_tile(1, 1);
        }
        for (int tl = 0; tl < nt2; ++tl) {
            if (!RES) __syncthreads();
            if (KB && tl == (nt2 >> 1)) at_mid();
            const bool have_next = tl + 1 < nt2;
            if (!RES && tl + 2 < nt2) g2r_tile(tl + 2);
            const float* T = tile_ptr(tl + 1);
            const int j = (ch * nt2 + tl) * 32 + l31;
            const float xxc = RES ? cxx[j] : hcxx[(tl % 3) * 32 + l31];
            float bf[2][APX ? 1 : GS];
            kbf16x8 bh, bl, bhn, bln;                       // APX: fragments of the current / the next channel block of the next tile
            if (have_next) {
                if (APX) {
                    fragA((tl + 1) & 1, 0, bhn, bln);
                } else {
#pragma unroll
                    for (int s = 0; s < GS; ++s) bf[0][s] = T[(2 * s) * KM_STRIDE];
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) accNext[r] = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (APX) {
                    // the 3 NKB bf16 MFMAs of the next tile spread over the 16 query rows of the select loop: MFMA m = block m / 3,
                    // product m % 3 (hi hi, hi lo, lo hi); a block's fragments are read one block ahead
                    if (have_next) {
                        constexpr int M = 3 * NKB;
#pragma unroll
                        for (int m = (r * M) / 16; m < ((r + 1) * M) / 16; ++m) {
                            const int kb = m / 3, w = m % 3;
                            if (w == 0) {
                                bh = bhn; bl = bln;
                                if (kb + 1 < NKB) fragA((tl + 1) & 1, kb + 1, bhn, bln);
                            }
                            accNext = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w == 2 ? qlo[kb] : qhi[kb], w == 1 ? bl : bh, accNext, 0, 0, 0);
                        }
                    }
                } else
                if (have_next) {
                    if (NSTEP >= 16) {
                        const int s0 = r * SPR, g = s0 / GS;
                        if (s0 % GS == 0 && g + 1 < NG) {
#pragma unroll
                            for (int s = 0; s < GS; ++s) bf[(g + 1) & 1][s] = T[(2 * ((g + 1) * GS + s)) * KM_STRIDE];
                        }
#pragma unroll
                        for (int u = 0; u < SPR; ++u)
                            accNext = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[s0 + u], bf[g & 1][(s0 + u) % GS], accNext, 0, 0, 0);
                    } else if (r < NSTEP) {
                        accNext = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[r], bf[0][r], accNext, 0, 0, 0);
                    }
                }
                const float pd = fmaf(2.0f, accCur[r], -xxc) - xxq[r];
                sel(r, pd, j);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (!RES && tl + 2 < nt2) { if (APX) r2s_tileA(tl & 1, tl + 2); else r2s_tile(tl & 1, tl + 2); }
#pragma unroll
            for (int r = 0; r < 16; ++r) accCur[r] = accNext[r];
        }
    };

    // ---- pass A: chunk maxima of this half
    {
        float cm[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) cm[r] = -INFINITY;
        sweep([&](int r, float pd, int) { cm[r] = fmaxf(cm[r], pd); },
              [&]() {          // KB: the first half's maxima go straight to the exchange image (bufk is dead during pass A)
                  if (KB) {
#pragma unroll
                      for (int r = 0; r < 16; ++r) {
                          xch[(((qg * 2 + ch) * 2 + 0) * 16 + r) * KNN5_XS + lane] = cm[r];
                          cm[r] = -INFINITY;
                      }
                  }
              }, std::true_type{});
#pragma unroll
        for (int r = 0; r < 16; ++r) xch[(KB ? ((qg * 2 + ch) * 2 + 1) * 16 + r : (qg * 2 + ch) * 16 + r) * KNN5_XS + lane] = cm[r];
    }
    __syncthreads();
    // tau = k-th largest of a query's chunk maxima.  One lane per query: the first 32 lanes of waves 0-3 (one per
    // SIMD) pull the 64 values of "their" query into registers and run a bitonic sorting network (672 min/max pairs,
    // no cross-lane traffic, no data-dependent control).  KB = 1: lanes 32-63 sort the 64 maxima of the other candidate
    // half at the same time, then the two sorted runs are merged (header comment).
    if (ch == 0 && (KB || lane < 32)) {
        const int r = (l31 & 3) + 4 * (l31 >> 3), hq = (l31 >> 2) & 1;     // l31 = query row of the group
        float v[64];
        if (KB) {
#pragma unroll
            for (int c = 0; c < 2; ++c)                                    // c = part (first / second half of the tiles); h = candidate half
#pragma unroll
                for (int i4 = 0; i4 < 8; ++i4) {
                    const f32x4 t = *(const f32x4*)(xch + (((qg * 2 + h) * 2 + c) * 16 + r) * KNN5_XS + hq * 32 + 4 * i4);
                    v[c * 32 + 4 * i4 + 0] = t[0]; v[c * 32 + 4 * i4 + 1] = t[1];
                    v[c * 32 + 4 * i4 + 2] = t[2]; v[c * 32 + 4 * i4 + 3] = t[3];
                }
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int i4 = 0; i4 < 8; ++i4) {
                    const f32x4 t = *(const f32x4*)(xch + ((qg * 2 + c) * 16 + r) * KNN5_XS + hq * 32 + 4 * i4);
                    v[c * 32 + 4 * i4 + 0] = t[0]; v[c * 32 + 4 * i4 + 1] = t[1];
                    v[c * 32 + 4 * i4 + 2] = t[2]; v[c * 32 + 4 * i4 + 3] = t[3];
                }
        }
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
        if (KB) {
            // top 64 of the two descending runs (mine and my partner lane's, lane ^ 32): t[i] = max(a[i], b[63-i]) is bitonic
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const float pa = __shfl_xor(v[63 - i], 32, 64), pb = __shfl_xor(v[i], 32, 64);
                v[i] = fmaxf(v[i], pa);
                v[63 - i] = fmaxf(v[63 - i], pb);
            }
#pragma unroll
            for (int j = 32; j > 0; j >>= 1)
#pragma unroll
                for (int i = 0; i < 64; ++i) {
                    const int l = i ^ j;
                    if (l > i) {
                        const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
                        v[i] = hi; v[l] = lo;
                    }
                }
        }
        float t = v[0];
#pragma unroll
        for (int i = 1; i < (KB ? 64 : 32); ++i) t = (i == k - 1) ? v[i] : t;
        if (!KB || h == 0) tau[(qg * 16 + r) * 2 + hq] = t;
    }
    if (KB && tid < 128) cnts[tid] = 0;
    __syncthreads();                           // tau complete; xch (aliases bufk) is dead from here on
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        thr[r] = tau[(qg * 16 + r) * 2 + h];
        if (AP) {                              // approximate pass A: lower the bound by the distance error of this query (header comment)
            const float t = thr[r] - KNN5_EPS * (xxq[r] + xxmax);
            thr[r] = t == t ? t : -INFINITY;
        }
    }
    if (KB || AP) load_queries();              // dead across pass A / the tau phase (register budget), read here

    if (!KB) {
        // ---- pass B: survivors of this half -> this wave's key buffers
        u64* mybuf = bufk + (size_t)(qg * 2 + ch) * 32 * KNN5_CAP;
        int cnt[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) cnt[r] = 0;
        sweep([&](int r, float pd, int j) {
            const bool pass = pd >= thr[r];
            const unsigned long long m = __ballot(pass);
            if (m) {
                const unsigned mine = h ? (unsigned)(m >> 32) : (unsigned)m;
                const int pos = cnt[r] + __builtin_popcount(mine & ((1u << l31) - 1u));
                if (pass && pos < KNN5_CAP) mybuf[((r & 3) + 8 * (r >> 2) + 4 * h) * KNN5_CAP + pos] = knn_key(pd, j);
                cnt[r] += __builtin_popcount(mine);
            }
        }, []() {}, std::false_type{});
        bool over = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) over |= cnt[r] > KNN5_CAP;

        if (__syncthreads_or(over ? 1 : 0)) {
            // ---- pass C (exact for any input): sequential insertion over this half, lane-distributed sorted lists
            float lv[16];
            int li[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) { lv[r] = -INFINITY; li[r] = 0x7fffffff; thr[r] = -INFINITY; }
            sweep([&](int r, float pd, int j) {
                unsigned long long m = __ballot(pd > thr[r]);
                if (m) {
                    unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
                    const int pdi = __float_as_int(pd);
                    const int jbase = j - l31;
                    while (lo | hi) {
                        const int s0 = lo ? __builtin_ctz(lo) : 0, s1 = hi ? __builtin_ctz(hi) : 0;
                        const float x0 = __int_as_float(__builtin_amdgcn_readlane(pdi, s0));
                        const float x1 = __int_as_float(__builtin_amdgcn_readlane(pdi, 32 + s1));
                        const bool active = h ? (hi != 0) : (lo != 0);
                        const float xv = h ? x1 : x0;
                        const int xj = jbase + (h ? s1 : s0);
                        const float upv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(lv[r]), 0x138, 0xf, 0xf, false));
                        const int upi = __builtin_amdgcn_update_dpp(0, li[r], 0x138, 0xf, 0xf, false);
                        const bool lt = lv[r] < xv;
                        const bool uplt = (l31 > 0) && (upv < xv);
                        if (active && lt) { lv[r] = uplt ? upv : xv; li[r] = uplt ? upi : xj; }
                        lo &= lo - 1; hi &= hi - 1;
                    }
                    const float t0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lv[r]), k - 1));
                    const float t1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lv[r]), 32 + k - 1));
                    thr[r] = h ? t1 : t0;
                }
            }, []() {}, std::false_type{});
            // a half with fewer than k candidates (N/2 < k) leaves -inf/0x7fffffff fillers: they are not published
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool valid = l31 < k && li[r] != 0x7fffffff;
                if (valid) mybuf[((r & 3) + 8 * (r >> 2) + 4 * h) * KNN5_CAP + l31] = knn_key(lv[r], li[r]);
                const unsigned long long m = __ballot(valid);
                cnt[r] = __builtin_popcount(h ? (unsigned)(m >> 32) : (unsigned)m);
            }
        }
        if (l31 == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) cnts[(qg * 2 + ch) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = cnt[r];
        }
        __syncthreads();

        // ---- final: exact rank among the <= 64 keys of a query; this wave finishes 8 of the group's 16 rows
        for (int rr = 0; rr < 8; ++rr) {
            const int r = ch * 8 + rr;
            const int qrow = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int n0 = cnts[(qg * 2 + 0) * 32 + qrow], n1 = cnts[(qg * 2 + 1) * 32 + qrow];
            const u64* K0 = bufk + ((size_t)(qg * 2 + 0) * 32 + qrow) * KNN5_CAP;
            const u64* K1 = bufk + ((size_t)(qg * 2 + 1) * 32 + qrow) * KNN5_CAP;
            const u64 m0 = l31 < n0 ? K0[l31] : 0ull, m1 = l31 < n1 ? K1[l31] : 0ull;
            int nm = max(n0, n1);
            nm = max(__builtin_amdgcn_readlane(nm, 0), __builtin_amdgcn_readlane(nm, 32));
            int rank0 = 0, rank1 = 0;
            for (int i = 0; i < nm; i += 2) {
                const u32x4 p0 = *(const u32x4*)(K0 + i), p1 = *(const u32x4*)(K1 + i);
                const u64 a0 = i < n0 ? ((u64)p0[1] << 32 | p0[0]) : 0ull, a1 = i + 1 < n0 ? ((u64)p0[3] << 32 | p0[2]) : 0ull;
                const u64 c0 = i < n1 ? ((u64)p1[1] << 32 | p1[0]) : 0ull, c1 = i + 1 < n1 ? ((u64)p1[3] << 32 | p1[2]) : 0ull;
                rank0 += (a0 > m0) + (a1 > m0) + (c0 > m0) + (c1 > m0);
                rank1 += (a0 > m1) + (a1 > m1) + (c0 > m1) + (c1 > m1);
            }
            int* out = idx + ((size_t)b * N + q0 + qrow) * k;
            if (l31 < n0 && rank0 < k) out[rank0] = ~(int)(unsigned)m0;
            if (l31 < n1 && rank1 < k) out[rank1] = ~(int)(unsigned)m1;
        }
    } else {
    // ================= KB = 1: 32 < k <= 64 =================
    // ---- pass B: survivors of BOTH halves -> the query's one key buffer (LDS counter per query)
    sweep([&](int r, float pd, int j) {
        const bool pass = pd >= thr[r];
        const unsigned long long m = __ballot(pass);
        if (m) {
            const unsigned mine = h ? (unsigned)(m >> 32) : (unsigned)m;      // hits of my query row (uniform over the half-wave)
            if (mine) {
                const int qrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int leader = __builtin_ctz(mine);
                int base = 0;
                if (l31 == leader) base = atomicAdd(&cnts[qg * 32 + qrow], __builtin_popcount(mine));
                base = __shfl(base, (h << 5) + leader, 64);
                const int pos = base + __builtin_popcount(mine & ((1u << l31) - 1u));
                if (pass && pos < KNN5_CAPT) bufk[(size_t)(qg * 32 + qrow) * KNN5_CAPT + pos] = knn_key(pd, j);
            }
        }
    }, []() {}, std::false_type{});
    __syncthreads();
    const bool over = tid < 128 && cnts[tid] > KNN5_CAPT;
    if (__syncthreads_or(over ? 1 : 0)) {
        // ---- pass C (exact for any input): sequential insertion over this half; the sorted list of a query row lives in
        // the 32 lanes of its half-wave with TWO entries per lane: positions l31 (lvA) and 32 + l31 (lvB).  An insertion into
        // the first level pushes its last element (lane 31's) into the second.
        float lvA[16], lvB[16];
        int liA[16], liB[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) { lvA[r] = lvB[r] = -INFINITY; liA[r] = liB[r] = 0x7fffffff; }
        sweep([&](int r, float pd, int j) {
            // current k-th best of my query row = list position k - 1 (first level: lane k - 1; second level: lane k - 33); read
            // from the list itself instead of keeping 16 more live registers
            const int tsrc = __float_as_int(k <= 32 ? lvA[r] : lvB[r]), tl = (k - 1) & 31;
            const float t0 = __int_as_float(__builtin_amdgcn_readlane(tsrc, tl));
            const float t1 = __int_as_float(__builtin_amdgcn_readlane(tsrc, 32 + tl));
            unsigned long long m = __ballot(pd > (h ? t1 : t0));
            if (m) {
                unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
                const int pdi = __float_as_int(pd);
                const int jbase = j - l31;
                while (lo | hi) {
                    const int s0 = lo ? __builtin_ctz(lo) : 0, s1 = hi ? __builtin_ctz(hi) : 0;
                    const float x0 = __int_as_float(__builtin_amdgcn_readlane(pdi, s0));
                    const float x1 = __int_as_float(__builtin_amdgcn_readlane(pdi, 32 + s1));
                    const bool active = h ? (hi != 0) : (lo != 0);
                    const float xv = h ? x1 : x0;
                    const int xj = jbase + (h ? s1 : s0);
                    // the element that leaves the first level if xv enters it: the current last one (lane 31 of my half)
                    const float c0v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lvA[r]), 31));
                    const float c1v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lvA[r]), 63));
                    const int c0i = __builtin_amdgcn_readlane(liA[r], 31), c1i = __builtin_amdgcn_readlane(liA[r], 63);
                    const float lastv = h ? c1v : c0v;
                    const int lasti = h ? c1i : c0i;
                    const bool intoA = lastv < xv;
                    const float yv = intoA ? lastv : xv;               // what the second level receives
                    const int yj = intoA ? lasti : xj;
                    {
                        const float upv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(lvA[r]), 0x138, 0xf, 0xf, false));
                        const int upi = __builtin_amdgcn_update_dpp(0, liA[r], 0x138, 0xf, 0xf, false);
                        const bool lt = lvA[r] < xv;
                        const bool uplt = (l31 > 0) && (upv < xv);
                        if (active && lt) { lvA[r] = uplt ? upv : xv; liA[r] = uplt ? upi : xj; }
                    }
                    {   // an element pushed out of the first level precedes EVERYTHING in the second (it was ahead of it in the total
                        // order, ties included): it becomes position 32 and the whole level shifts; a fresh candidate is inserted
                        // behind its equals like in the first level
                        const float upv = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(lvB[r]), 0x138, 0xf, 0xf, false));
                        const int upi = __builtin_amdgcn_update_dpp(0, liB[r], 0x138, 0xf, 0xf, false);
                        const bool lt = intoA || lvB[r] < yv;
                        const bool uplt = (l31 > 0) && (intoA || upv < yv);
                        if (active && lt) { lvB[r] = uplt ? upv : yv; liB[r] = uplt ? upi : yj; }
                    }
                    lo &= lo - 1; hi &= hi - 1;
                }
            }
        }, []() {}, std::false_type{});
        // Each half now holds its exact top-k per query (fewer when N/2 < k: fillers are not published).  The halves publish
        // one after the other through the query's buffer; the other half ranks its own keys against what it reads.
        // keys are rebuilt from (value, index) where they are used: 0 = no key (every real key is > 0)
#define KNN5_KEYA(r) (liA[r] != 0x7fffffff ? knn_key(lvA[r], liA[r]) : 0ull)
#define KNN5_KEYB(r) ((32 + l31 < k && liB[r] != 0x7fffffff) ? knn_key(lvB[r], liB[r]) : 0ull)
        for (int turn = 0; turn < 2; ++turn) {
            __syncthreads();                                   // everyone is done with the buffer's previous content
            if (ch == turn) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    u64* K = bufk + (size_t)(qg * 32 + (r & 3) + 8 * (r >> 2) + 4 * h) * KNN5_CAPT;
                    K[l31] = KNN5_KEYA(r);
                    K[32 + l31] = KNN5_KEYB(r);
                }
            }
            __syncthreads();
            if (ch != turn) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qrow = (r & 3) + 8 * (r >> 2) + 4 * h;
                    const u64* K = bufk + (size_t)(qg * 32 + qrow) * KNN5_CAPT;
                    const u64 kA = KNN5_KEYA(r), kB = KNN5_KEYB(r);
                    int ra = l31, rb = 32 + l31;               // rank inside my own sorted list
                    for (int i = 0; i < 64; i += 2) {
                        const u32x4 p = *(const u32x4*)(K + i);
                        const u64 a0 = (u64)p[1] << 32 | p[0], a1 = (u64)p[3] << 32 | p[2];
                        ra += (a0 > kA) + (a1 > kA);
                        rb += (a0 > kB) + (a1 > kB);
                    }
                    int* out = idx + ((size_t)b * N + q0 + qrow) * k;
                    if (kA != 0ull && ra < k) out[ra] = ~(int)(unsigned)kA;
                    if (kB != 0ull && rb < k) out[rb] = ~(int)(unsigned)kB;
                }
            }
        }
#undef KNN5_KEYA
#undef KNN5_KEYB
        return;
    }
    // ---- final: exact rank among the <= CAPT keys of a query; this wave finishes 8 of the group's 16 rows
    for (int rr = 0; rr < 8; ++rr) {
        const int r = ch * 8 + rr;
        const int qrow = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int n = cnts[qg * 32 + qrow];
        const u64* K = bufk + (size_t)(qg * 32 + qrow) * KNN5_CAPT;
        const u64 m0 = l31 < n ? K[l31] : 0ull, m1 = 32 + l31 < n ? K[32 + l31] : 0ull, m2 = 64 + l31 < n ? K[64 + l31] : 0ull;
        int nm = max(__builtin_amdgcn_readlane(n, 0), __builtin_amdgcn_readlane(n, 32));
        int rank0 = 0, rank1 = 0, rank2 = 0;
        for (int i = 0; i < nm; i += 2) {
            const u32x4 p = *(const u32x4*)(K + i);
            const u64 a0 = i < n ? ((u64)p[1] << 32 | p[0]) : 0ull, a1 = i + 1 < n ? ((u64)p[3] << 32 | p[2]) : 0ull;
            rank0 += (a0 > m0) + (a1 > m0);
            rank1 += (a0 > m1) + (a1 > m1);
            rank2 += (a0 > m2) + (a1 > m2);
        }
        int* out = idx + ((size_t)b * N + q0 + qrow) * k;
        if (l31 < n && rank0 < k) out[rank0] = ~(int)(unsigned)m0;
        if (32 + l31 < n && rank1 < k) out[rank1] = ~(int)(unsigned)m1;
        if (64 + l31 < n && rank2 < k) out[rank2] = ~(int)(unsigned)m2;
    }
    }
}

template <int CT, bool VEC, bool RES, int KB>
static int launch_knn_mfma5_ct(hipStream_t st, const float* x, int ld, const float* xx, int B, int N, int C, int k, int* idx,
                               size_t lds, const int* only, bool dry) {
    if (dry) return 0;
    if (lds > 64 * 1024) {
        hipError_t e = mlsp_lds_limit((const void*)knn_mfma5_kernel<CT, VEC, RES, KB>, lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((knn_mfma5_kernel<CT, VEC, RES, KB>), dim3((N / 128) * B), dim3(512), lds, st, x, xx, ld, N, C, k, idx, B, only);
    return mlsp_launch_status();
}

static size_t knn5_lds_bytes(int CT, int N, bool res, bool kb, bool vec = false) {
    size_t tile = (size_t)CT * KM_STRIDE;
    if ((CT == 64 || (CT == 128 && !kb)) && !res && vec && (size_t)32 * (CT + 8) > tile) tile = (size_t)32 * (CT + 8);     // pass-A images (kernel: TILE_ALLOC)
    const size_t keys = kb ? (size_t)2 * 128 * KNN5_CAPT : (size_t)2 * 4 * 2 * 32 * KNN5_CAP;     // floats
    const size_t fl = (res ? (size_t)(N / 32) * tile + N : 4 * tile + 192) + keys + 128 + 256;
    return fl * sizeof(float);
}

// returns MLSP_ERR_UNSUPPORTED when the shape is outside v5's fast path (caller falls back to v4 / the list-merge kernel).
// only: per-cloud flags (device), nullptr = every cloud; dry: launch nothing, just say whether the shape is taken
static int launch_knn_mfma5(hipStream_t st, const float* x, int ld, const float* xx, int B, int N, int C, int k, int* idx,
                            const int* only = nullptr, bool dry = false) {
    if (N % 128 != 0 || k > 64 || C > 128) return MLSP_ERR_UNSUPPORTED;
    const bool kb = k > 24;        // k = 25..32 on the 64-maxima bound overflow its 32-key buffers too often (734 us vs 290 at N = 2048)
    const int CT = C <= 4 ? 4 : C <= 16 ? 16 : C <= 64 ? 64 : 128;
    const bool vec = (C == CT) && (ld % 4 == 0) && (((uintptr_t)x & 15) == 0);
    const bool res = CT <= 16 && knn5_lds_bytes(CT, N, true, kb) <= 160 * 1024;
    const size_t lds = knn5_lds_bytes(CT, N, res, kb, vec);
    if (lds > 160 * 1024) return MLSP_ERR_UNSUPPORTED;
#define KNN5_GO(CTV, VECV, RESV) do { if (kb) return launch_knn_mfma5_ct<CTV, VECV, RESV, 1>(st, x, ld, xx, B, N, C, k, idx, lds, only, dry); \
                                      return launch_knn_mfma5_ct<CTV, VECV, RESV, 0>(st, x, ld, xx, B, N, C, k, idx, lds, only, dry); } while (0)
    if (CT == 4) { if (res) { if (vec) KNN5_GO(4, true, true); KNN5_GO(4, false, true); } if (vec) KNN5_GO(4, true, false); KNN5_GO(4, false, false); }
    if (CT == 16) { if (res) { if (vec) KNN5_GO(16, true, true); KNN5_GO(16, false, true); } if (vec) KNN5_GO(16, true, false); KNN5_GO(16, false, false); }
    if (CT == 64) { if (vec) KNN5_GO(64, true, false); KNN5_GO(64, false, false); }
    if (vec) KNN5_GO(128, true, false);
    if (kb) return MLSP_ERR_UNSUPPORTED;       // k > 24 with 64 < C < 128 or unaligned rows: out of registers, stays on the list-merge kernel
    return launch_knn_mfma5_ct<128, false, false, 0>(st, x, ld, xx, B, N, C, k, idx, lds, only, dry);
#undef KNN5_GO
}

static size_t knn_lds_bytes(int KMAX, int C, bool runtime_c) {
    size_t tiles = (size_t)4 * KNN_TJ * C + 4 * KNN_TJ + (runtime_c ? (size_t)KNN_QB * (C + 1) : 0);
    size_t merge = (size_t)3 * KMAX * 64 * 2;
    return (tiles > merge ? tiles : merge) * sizeof(float);
}

template <int KMAX>
static int launch_knn_k(hipStream_t st, const float* x, int ld, const float* xx, int B, int N, int C, int k, int* idx) {
    dim3 grid((N + KNN_QB - 1) / KNN_QB, B), block(256);
    if (C == 3) {
        hipLaunchKernelGGL((knn_kernel<KMAX, 3>), grid, block, knn_lds_bytes(KMAX, 3, false), st, x, xx, ld, N, C, k, idx);
    } else {
        size_t lds = knn_lds_bytes(KMAX, C, true);
        if (lds > 160 * 1024) return MLSP_ERR_UNSUPPORTED;
        if (lds > 64 * 1024) {
            hipError_t e = mlsp_lds_limit((const void*)knn_kernel<KMAX, 0>, lds);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL((knn_kernel<KMAX, 0>), grid, block, lds, st, x, xx, ld, N, C, k, idx);
    }
    return mlsp_launch_status();
}

// xx_ws: [B*N] floats of workspace; planes (nullable): knn6_plane_bytes(B*N, C) bytes of workspace for the v6 kernel's bf16 images
int launch_knn(hipStream_t st, const float* x, int ld, int B, int N, int C, int k, int* idx, float* xx_ws, void* planes, size_t plane_bytes) {
    if (!x || !idx || !xx_ws || B <= 0 || N <= 0 || C <= 0 || k <= 0 || k > N || ld < C) return MLSP_ERR_ARG;
    int P = B * N;
    // C <= 3 (raw and transformed cloud): the v6 skeleton with vector-exact sweeps (knn6.hip VEX)
    if (planes && knn6_vex_supported(B, N, C, k) && plane_bytes >= knn6_vex_bytes(P)) {
        const int rc = launch_knn6_vex(st, x, ld, B, N, C, k, idx, xx_ws, planes);
        if (rc != MLSP_ERR_UNSUPPORTED) return rc;
    }
    // v6 (knn6.hip): k <= 24 on whole 128-query chunks -- the five graph stages of DGCNN
    if (planes && knn6_supported(B, N, C, k) && plane_bytes >= knn6_plane_bytes(P, C) && C > 16) {   // (C <= 16 stays on v5 until v6's selection phases beat it there)
        const int rc = launch_knn6(st, x, ld, B, N, C, k, idx, xx_ws, planes);
        if (rc != MLSP_ERR_UNSUPPORTED) return rc;
    }
    // 24 < k <= 40 (PointSegDA's k = 40): the wide v6 kernel, with the v5 kernel behind it for the clouds it flags (list overflow: massive
    // ties; non-finite bounds) -- v5's workgroups of unflagged clouds return at once.  Only where v5 itself takes the shape.
    // Every C <= 128: at C = 3 (B = 16, N = 2048, k = 40) 82 us against v5's 117, C = 64 152 / 235, C = 128 210 / 435.
    if (planes && knn6w_supported(B, N, C, k) && plane_bytes >= knn6_plane_bytes(P, C) &&
        launch_knn_mfma5(st, x, ld, xx_ws, B, N, C, k, idx, nullptr, true) == 0) {
        int* flags = nullptr;
        const int rc = launch_knn6w(st, x, ld, B, N, C, k, idx, xx_ws, planes, &flags);
        if (rc == 0) return launch_knn_mfma5(st, x, ld, xx_ws, B, N, C, k, idx, flags, false);
        if (rc != MLSP_ERR_UNSUPPORTED) return rc;
    }
    hipLaunchKernelGGL(sqnorm_kernel, dim3((P + 255) / 256), dim3(256), 0, st, x, ld, P, C, xx_ws, idx, k);
    // matrix-core kernels for every C <= 256 (the widest graph stage of the reference is 128 channels); beyond that only what the
    // VALU kernel's LDS tiles hold (C <= ~200 at k <= 40): MLSP_ERR_UNSUPPORTED otherwise
    if (C <= 256) {
        // two-pass threshold select pays once there are enough candidates per query; small clouds keep v3
        if (k <= 32 && C <= 128 && N >= 256) {
            const int rc = launch_knn_mfma5(st, x, ld, xx_ws, B, N, C, k, idx);
            if (rc != MLSP_ERR_UNSUPPORTED) return rc;
            return launch_knn_mfma4(st, x, ld, xx_ws, B, N, C, k, idx);
        }
        if (k > 24 && k <= 64 && C <= 128 && N >= 128) {       // 128 chunk maxima per query need N >= 128
            const int rc = launch_knn_mfma5(st, x, ld, xx_ws, B, N, C, k, idx);
            if (rc != MLSP_ERR_UNSUPPORTED) return rc;
        }
        if (k <= 32) return launch_knn_mfma3(st, x, ld, xx_ws, B, N, C, k, idx);      // lane-distributed lists
        // 32 < k <= 40 on a shape the two-pass kernel does not take (ragged N, N < 128, 64 < C < 128 or C > 128): the VALU kernel
    }
    if (k <= 20) return launch_knn_k<20>(st, x, ld, xx_ws, B, N, C, k, idx);
    if (k <= 40) return launch_knn_k<40>(st, x, ld, xx_ws, B, N, C, k, idx);
    return MLSP_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------------
// Reverse neighbour index (CSR of the transposed kNN graph), one workgroup per cloud.
// For every point j: the list of (i, slot) with idx[i][slot] == j, sorted by i*256+slot so that the
// backward gather-reduce that walks it sums in a fixed order (bitwise reproducible gradients).
//   rev_off [B*N+1]  global edge offsets;  rev_ent [B*N*k]  packed (i_local << 8 | slot)
#define RV_SPLIT_MAX 16                   // workgroups per cloud: 8, or 16 when 8 would leave CUs idle (chosen by the launcher)
#define RV_CAP (16 * 1024)                // LDS entries of a slice's lists, twice: filled / ordered (a slice past that sorts in place in global memory)
// `nsplit` workgroups per cloud, each owns a contiguous slice of the destinations: it counts only the edges that point into its
// slice (LDS atomics are the expensive instruction here: ~3 clocks per lane), gets the slice's base offset by counting the edges
// that point BELOW it (plain adds + one block reduction), fills its lists and orders every list.
// skip_pad: the padding slots of a ball-query group (copies of its first hit: slot s > 0 with idx[i][s] == idx[i][0]) are left out of the
// lists -- their rows are identical, the consumer adds them as a multiple of one row (sa.hip, sa_fold_bwd_point_kernel).  The lists of a
// cloud then no longer fill its E entries, so the list LENGTHS are returned as well (rev_cnt, nullable otherwise).
typedef int knn_i32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(1024) void knn_reverse_kernel(const int* __restrict__ idx, int N, int k,
                                                           int* __restrict__ rev_off, int* __restrict__ rev_ent,
                                                           int B, int S, int nsplit, int skip_pad, int* __restrict__ rev_cnt) {
    extern __shared__ __attribute__((aligned(16))) int ism[];
    __shared__ int wsum[16];
    __shared__ int nbig;                  // lists of more than 64 entries: queued (cnt is free by then) for the whole-workgroup loop
    int b, part;
    xcd_cloud_map(blockIdx.x, nsplit, B, b, part);        // the workgroups of a cloud share an XCD (they read the same idx)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int dper = (N + nsplit - 1) / nsplit, d0 = min(N, part * dper), d1 = min(N, d0 + dper), nd = d1 - d0;
    int* cnt = ism;            // [dper]
    int* off = ism + dper;     // [dper + 1]  offsets inside the slice
    int* offp = off + dper + 1;   // [dper + 1]  the same with every list padded to a multiple of 4 entries: where the lists lie in `lent`
    int* lent = ism + ((3 * dper + 2 + 3) & ~3);   // [RV_CAP] as filled; 16-byte aligned lists (pads hold INT_MAX): the ordering reads four entries per LDS instruction
    int* lord = lent + RV_CAP;    // [RV_CAP] ordered (unpadded: the slice's part of rev_ent)
    // S source rows of k slots per cloud point at N destinations (S == N for the kNN graph; the set-abstraction grouping has
    // S sampled centres gathering from N points)
    const int* ib = idx + (size_t)b * S * k;
    const int E = S * k;
    for (int j = tid; j < nd; j += nt) cnt[j] = 0;
    if (tid == 0) nbig = 0;
    __syncthreads();
    int below = 0;
    // RV_B index loads in flight per thread (the atomics would serialise them): a pass is a chain of ceil(E / (RV_B nt)) load latencies, ONE
    // at the DGCNN shape (E = 20 Ki entries, 1024 threads) -- and then the fill pass below reuses the registers instead of reading idx again
    constexpr int RV_B = 20;
    const bool one_trip = E <= nt * RV_B;
    // Several trips (PointSegDA: N = 2048, k = 40 -> 80 entries per thread): the entries that fall into this workgroup's slice (E / nsplit of
    // them on average) are COMPACTED into `lord` as (destination, source entry) pairs while they are counted -- `lord` is free until the
    // lists are ordered -- and the fill pass walks those pairs instead of scanning the cloud's E indices again.  More than RV_CAP / 2 pairs:
    // the fill pass scans again as before.
    __shared__ int ncomp;
    if (tid == 0) ncomp = 0;
    const int comp_cap = RV_CAP / 2;
    int jk[RV_B];
    __syncthreads();
    for (int eb = tid; eb < E; eb += nt * RV_B) {
#pragma unroll
        for (int u = 0; u < RV_B; ++u) jk[u] = eb + u * nt < E ? ib[eb + u * nt] : -1;
#pragma unroll
        for (int u = 0; u < RV_B; ++u) {
            int j = jk[u];
            if (skip_pad && j >= 0) { const int e = eb + u * nt, sl = e % k; if (sl != 0 && j == ib[e - sl]) j = -1; }
            jk[u] = j;
            below += j >= 0 && j < d0;
            const bool mine = j >= d0 && j < d1;
            if (mine) atomicAdd(&cnt[j - d0], 1);
            if (!one_trip) {                             // (uniform) one LDS atomic per wave and entry slot: the wave's matches take consecutive places
                const unsigned long long mm = __ballot(mine);
                if (mm) {
                    const int lane_ = tid & 63;
                    int base_ = 0;
                    if (lane_ == 0) base_ = atomicAdd(&ncomp, __builtin_popcountll(mm));
                    base_ = __shfl(base_, 0, 64);
                    const int at = base_ + __builtin_popcountll(mm & ((1ull << lane_) - 1ull));
                    if (mine && at < comp_cap) { lord[2 * at] = j - d0; lord[2 * at + 1] = eb + u * nt; }
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = below;
    __syncthreads();
    int s0 = 0;
    for (int w = 0; w < (nt >> 6); ++w) s0 += wsum[w];   // edges into the slices before this one
    // exclusive scan of the slice's counts by one wave
    if (tid < 64) {
        const int chunk = (nd + 63) / 64;
        const int beg = min(nd, tid * chunk), end = min(nd, beg + chunk);
        int sm = 0, smp = 0;
        for (int j = beg; j < end; ++j) { sm += cnt[j]; smp += (cnt[j] + 3) & ~3; }
        int incl = sm, inclp = smp;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64), tp = __shfl_up(inclp, o, 64);
            if (tid >= o) { incl += t; inclp += tp; }
        }
        int run = incl - sm, runp = inclp - smp;
        for (int j = beg; j < end; ++j) { off[j] = run; run += cnt[j]; offp[j] = runp; runp += (cnt[j] + 3) & ~3; }
        if (tid == 63) { off[nd] = incl; offp[nd] = inclp; }
    }
    __syncthreads();
    const int gbase = b * E;
    const int sn = off[nd];
    const bool in_lds = offp[nd] <= RV_CAP;
    for (int j = tid; j < nd; j += nt) {
        rev_off[(size_t)b * N + d0 + j] = gbase + s0 + off[j];
        if (rev_cnt) rev_cnt[(size_t)b * N + d0 + j] = off[j + 1] - off[j];
        if (in_lds) {
            const int c = off[j + 1] - off[j];
            for (int q = c; q < ((c + 3) & ~3); ++q) lent[offp[j] + q] = 0x7fffffff;       // pads: never below a real entry
        }
        cnt[j] = 0;
    }
    if (b == B - 1 && part == nsplit - 1 && tid == 0) rev_off[(size_t)B * N] = gbase + E;
    __syncthreads();
    // fill + order this slice's lists in LDS, then one coalesced copy out: the ordering never touches global memory
    // (a slice with more than RV_CAP entries orders in place in global memory instead)
    int* ent = in_lds ? lent : rev_ent + gbase + s0;
    const int* eoff = in_lds ? offp : off;                                 // where list j starts in `ent`
    const bool compacted = !one_trip && in_lds && ncomp <= comp_cap;       // (ncomp == sn: every pair is there)
    if (compacted) {
        for (int i = tid; i < sn; i += nt) {
            const int jl = lord[2 * i], e = lord[2 * i + 1];
            const int pos = atomicAdd(&cnt[jl], 1);
            ent[eoff[jl] + pos] = ((e / k) << 8) | (e % k);
        }
    } else
    for (int eb = tid; eb < E; eb += nt * RV_B) {
        if (!one_trip) {
#pragma unroll
            for (int u = 0; u < RV_B; ++u) jk[u] = eb + u * nt < E ? ib[eb + u * nt] : -1;
        }
#pragma unroll
        for (int u = 0; u < RV_B; ++u) {
            int j = jk[u];
            const int e = eb + u * nt;
            if (!one_trip && skip_pad && j >= 0) { const int sl = e % k; if (sl != 0 && j == ib[e - sl]) j = -1; }
            if (j >= d0 && j < d1) {
                const int pos = atomicAdd(&cnt[j - d0], 1);
                ent[eoff[j - d0] + pos] = ((e / k) << 8) | (e % k);
            }
        }
    }
    __syncthreads();
    if (in_lds) {
        // order every list by (i, slot) by RANK: 16 lanes per list, every lane ranks its entries against the whole list (the 16 lanes
        // read the same LDS words: broadcasts) and writes them straight to their final place.  Lists of more than 64 entries
        // (ball-query groups are padded with copies of their first hit: a few points collect hundreds of edges) are left to the
        // second loop, where the whole workgroup shares one list.
        int* out = lord;
        const int lg = tid >> 4, ll = tid & 15;
        for (int j = lg; j < nd; j += nt >> 4) {
            const int e0 = off[j], n = off[j + 1] - e0;
            if (n > 64) {
                if (ll == 0) cnt[atomicAdd(&nbig, 1)] = j;
                continue;
            }
            const int* a = ent + offp[j];                  // 16-byte aligned, padded with INT_MAX to a multiple of 4
            for (int q = ll; q < n; q += 16) {
                const int v = a[q];
                int rank = 0;
                for (int e = 0; e < n; e += 4) {
                    const knn_i32x4 t = *(const knn_i32x4*)(a + e);
                    rank += (t[0] < v) + (t[1] < v) + (t[2] < v) + (t[3] < v);
                }
                out[e0 + rank] = v;
            }
        }
        __syncthreads();
        // lists of 65 .. 512 entries (the tail of a kNN graph's in-degree distribution: a dozen per workgroup at k = 40, a few at k = 20):
        // ONE WAVE per list, sixteen lists at a time -- the whole workgroup walking them one after the other was the longest phase of the
        // kernel (8 of 21 us at k = 20, 29 of 61 us at k = 40, N = 2048).  Longer ones (ball-query hubs): the whole workgroup per list.
        {
            const int wv = tid >> 6, ln = tid & 63;
            for (int bi = wv; bi < nbig; bi += nt >> 6) {
                const int j = cnt[bi];
                const int e0 = off[j], n = off[j + 1] - e0;
                if (n > 512) continue;
                const int* a = ent + offp[j];
                for (int q = ln; q < n; q += 64) {
                    const int v = a[q];
                    int rank = 0;
                    for (int e = 0; e < n; e += 4) {
                        const knn_i32x4 t = *(const knn_i32x4*)(a + e);
                        rank += (t[0] < v) + (t[1] < v) + (t[2] < v) + (t[3] < v);
                    }
                    out[e0 + rank] = v;
                }
            }
        }
        for (int bi = 0; bi < nbig; ++bi) {
            const int j = cnt[bi];
            const int e0 = off[j], n = off[j + 1] - e0;
            if (n <= 512) continue;
            const int* a = ent + offp[j];
            for (int q = tid; q < n; q += nt) {
                const int v = a[q];
                int rank = 0;
                for (int e = 0; e < n; ++e) rank += a[e] < v;
                out[e0 + rank] = v;
            }
        }
        __syncthreads();
        for (int i = tid; i < sn; i += nt) rev_ent[gbase + s0 + i] = lord[i];      // one coalesced copy out
        return;
    }
    __threadfence_block();
    // a slice too large for LDS: per-destination insertion sort in place in global memory
    for (int j = tid; j < nd; j += nt) {
        int* a = ent + off[j];
        const int n = off[j + 1] - off[j];
        for (int u = 1; u < n; ++u) {
            const int key = a[u];
            int w = u - 1;
            while (w >= 0 && a[w] > key) { a[w + 1] = a[w]; --w; }
            a[w + 1] = key;
        }
    }
}

static int launch_reverse(hipStream_t st, const int* idx, int B, int S, int N, int k, int* rev_off, int* rev_ent, int skip_pad = 0,
                          int* rev_cnt = nullptr) {
    if (!idx || !rev_off || !rev_ent || B <= 0 || N <= 0 || S <= 0 || k <= 0 || k > 256 || N > (1 << 22) || S > (1 << 22)) return MLSP_ERR_ARG;
    const int nsplit = B * 8 >= 256 || N < 1024 ? 8 : RV_SPLIT_MAX;
    const int dper = (N + nsplit - 1) / nsplit;
    const size_t lds = (size_t)(((3 * dper + 2 + 3) & ~3) + 2 * RV_CAP) * sizeof(int);
    if (lds > 160 * 1024) return MLSP_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        hipError_t e = mlsp_lds_limit((const void*)knn_reverse_kernel, lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(knn_reverse_kernel, dim3(B * nsplit), dim3(1024), lds, st, idx, N, k, rev_off, rev_ent, B, S, nsplit, skip_pad, rev_cnt);
    return mlsp_launch_status();
}

// ball-query groups (padded with copies of the first hit)
int launch_group_reverse(hipStream_t st, const int* idx, int B, int S, int N, int k, int* rev_off, int* rev_ent) {
    return launch_reverse(st, idx, B, S, N, k, rev_off, rev_ent);
}
// the same without the padding slots; pad_cnt [B*S] = number of padding slots of every group (s > 0 with idx[i][s] == idx[i][0])
__global__ __launch_bounds__(256) void group_pad_count_kernel(const int* __restrict__ idx, int G, int k, int* __restrict__ pad_cnt) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int* r = idx + (size_t)g * k;
    const int first = r[0];
    int c = 0;
    for (int s = 1; s < k; ++s) c += r[s] == first;
    pad_cnt[g] = c;
}
int launch_group_reverse_compact(hipStream_t st, const int* idx, int B, int S, int N, int k, int* rev_off, int* rev_cnt, int* rev_ent,
                                 int* pad_cnt) {
    if (!rev_cnt || !pad_cnt) return MLSP_ERR_ARG;
    const int rc = launch_reverse(st, idx, B, S, N, k, rev_off, rev_ent, 1, rev_cnt);
    if (rc != MLSP_OK) return rc;
    hipLaunchKernelGGL(group_pad_count_kernel, dim3((B * S + 255) / 256), dim3(256), 0, st, idx, B * S, k, pad_cnt);
    return mlsp_launch_status();
}
int launch_knn_reverse(hipStream_t st, const int* idx, int B, int N, int k, int* rev_off, int* rev_ent) {
    return launch_reverse(st, idx, B, N, N, k, rev_off, rev_ent);
}
