// Brute-force self-kNN in canonical arithmetic: the search kernels (v6's are in knn6.hip) and their one launcher, which follows knn_plan.h.
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
#include "knn_plan.h"      // KNN_QB / KNN_TJ, KM_STRIDE, the CAP constants, and which kernel a search of a given shape runs on
#include <type_traits>
#include <math.h>
#include <cstdlib>

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
// shapes run on the two-pass kernel, the few it does not take on the VALU kernel above.)  KM_STRIDE = 33: knn_plan.h.

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

// ------------------------------------------------------------------------------------------------
// v4: two-pass threshold select on top of the v3 tile pipeline (same canonical distances, same total order).
//   pass A  every lane keeps the running max of ITS column of the distance tiles (one v_max per value): 32 disjoint
//           chunk maxima per query.  The k-th largest of them, tau, is a lower bound of the k-th best distance (k
//           chunks each hold a value >= tau), so only candidates with pd >= tau can be in the answer (~30 of 1024).
//   pass B  recompute the tiles (the MFMA sweep is 20-60 us, the selection was 300); survivors are appended to a
//           per-query LDS buffer by ballot + prefix count -- no per-candidate loop.
//   final   exact rank of every survivor by counting (value desc, index asc): rank < k -> idx[q][rank].
// If any query of the workgroup overflows its 64-entry buffer (massive ties) the workgroup re-runs the v3
// sequential insertion (pass C), which is exact for any input.  (KNN4_CAP = 64: knn_plan.h)

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
// (KNN5_CAP = 32, KNN5_CAPT = 88: knn_plan.h)
#define KNN5_XS 68                // row stride (floats) of the pass-A exchange image: 16 B aligned rows, 2-way banked
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


// ------------------------------------------------------------------------------------------------
// The launcher.  knn_plan.h decides; a picker per family names every instantiation of its kernel once.
typedef void (*Knn1Fn)(const float*, const float*, int, int, int, int, int*);
typedef void (*Knn3Fn)(const float*, const float*, int, int, int, int, int, int*);
typedef void (*Knn4Fn)(const float*, const float*, int, int, int, int, int, int*, int);
typedef void (*Knn5Fn)(const float*, const float*, int, int, int, int, int*, int, const int*);

static Knn1Fn knn1_pick(int KMAX, int CT) {
    if (KMAX == 20) return CT == 3 ? knn_kernel<20, 3> : knn_kernel<20, 0>;
    return CT == 3 ? knn_kernel<40, 3> : knn_kernel<40, 0>;
}
static Knn3Fn knn3_pick(int CT) {
    return CT == 4 ? knn_mfma3_kernel<4> : CT == 16 ? knn_mfma3_kernel<16> : CT == 64 ? knn_mfma3_kernel<64> : CT == 128 ? knn_mfma3_kernel<128> : knn_mfma3_kernel<256>;
}
static Knn4Fn knn4_pick(int CT) {
    return CT == 4 ? knn_mfma4_kernel<4> : CT == 16 ? knn_mfma4_kernel<16> : CT == 64 ? knn_mfma4_kernel<64> : knn_mfma4_kernel<128>;
}
template <int CT, bool VEC, bool RES>
static Knn5Fn knn5_kb(bool kb) { return kb ? knn_mfma5_kernel<CT, VEC, RES, 1> : knn_mfma5_kernel<CT, VEC, RES, 0>; }
template <int CT, bool RES>
static Knn5Fn knn5_vec(const Knn5Plan& v) { return v.vec ? knn5_kb<CT, true, RES>(v.kb) : knn5_kb<CT, false, RES>(v.kb); }
static Knn5Fn knn5_pick(const Knn5Plan& v) {
    if (v.CT == 4) return v.res ? knn5_vec<4, true>(v) : knn5_vec<4, false>(v);
    if (v.CT == 16) return v.res ? knn5_vec<16, true>(v) : knn5_vec<16, false>(v);
    if (v.CT == 64) return knn5_vec<64, false>(v);
    if (v.vec) return knn5_kb<128, true, false>(v.kb);
    return knn_mfma5_kernel<128, false, false, 0>;          // (KB = 1 here is out of registers: the plan never asks for it)
}

bool knn6_vex_supported(int B, int N, int C, int k) { return knn_q_vex_supported(B, N, C, k); }
bool knn6_supported(int B, int N, int C, int k) { return knn_q_v6_supported(B, N, C, k); }
bool knn6w_supported(int B, int N, int C, int k) { return knn_q_v6w_supported(B, N, C, k); }

// xx_ws: [B*N] floats of workspace; planes (nullable): plane_bytes bytes of workspace for the v6 families (the plan's plane_bytes: the
// bf16 images of knn6_kernel / knn6w_kernel, the {x, xx} image of the vector-exact mode); a call the plan refuses launches nothing
int launch_knn(hipStream_t st, const float* x, int ld, int B, int N, int C, int k, int* idx, float* xx_ws, void* planes, size_t plane_bytes) {
    if (!x || !idx || !xx_ws) return MLSP_ERR_ARG;
    KnnAsk q;
    q.B = B; q.N = N; q.C = C; q.k = k; q.ld = ld; q.x16 = ((uintptr_t)x & 15) == 0;
    q.planes_avail = planes ? plane_bytes : 0; q.planes16 = ((uintptr_t)planes & 15) == 0;
    const KnnPlan p = knn_plan(q);
    if (p.status != MLSP_OK) return p.status;
    const int P = B * N;
    const dim3 grid(p.grid_x, p.grid_y), block(p.block);
    if (p.norm_pass) hipLaunchKernelGGL(sqnorm_kernel, dim3((P + 255) / 256), dim3(256), 0, st, x, ld, P, C, xx_ws, idx, k);
    switch (p.family) {
    case KNN_FAM_V5: return mlsp_launch_lds(st, knn5_pick(p.v5), grid, block, p.lds, x, xx_ws, ld, N, C, k, idx, B, nullptr);
    case KNN_FAM_V4: return mlsp_launch_lds(st, knn4_pick(p.CT), grid, block, p.lds, x, xx_ws, ld, N, C, k, (int)p.vec, idx, B);
    case KNN_FAM_V3: return mlsp_launch_lds(st, knn3_pick(p.CT), grid, block, p.lds, x, xx_ws, ld, N, C, k, (int)p.vec, idx);
    case KNN_FAM_VALU: return mlsp_launch_lds(st, knn1_pick(p.KMAX, p.CT), grid, block, p.lds, x, xx_ws, ld, N, C, k, idx);
    default: break;                                         // the v6 families: knn6.hip
    }
    int* flags = nullptr;
    const int rc = launch_knn6(st, p, x, ld, B, N, C, k, idx, xx_ws, planes, &flags);
    if (rc != MLSP_OK || p.family != KNN_FAM_V6W_V5) return rc;
    // the v5 kernel behind the wide one: its workgroups of unflagged clouds return at once
    return mlsp_launch_lds(st, knn5_pick(p.v5), dim3(p.v5.grid_x), dim3(512), p.v5.lds, x, xx_ws, ld, N, C, k, idx, B, flags);
}
