// Training-batch preparation (PointDA/data/dataloader.py:79-95, 136-149, 185-200: scale_to_unit_cube, rotate_shape, farthest_point_sample_np,
// random_rotate_one_axis, jitter_pointcloud) as ONE launch: one workgroup owns one cloud and never talks to another, no atomics, every loop
// bounded by the cloud's count or S.  The sampling loop is the skeleton of fps_kernel2 (sa.hip) -- cloud in LDS, points and running minima
// in registers, the arg-max one 64-bit key reduced by DPP inside a wave and through a double-buffered LDS slot across waves -- with a
// prologue (unit cube, pre-rotation) and an epilogue (post-rotation, jitter) whose arithmetic is batchprep_body.h's; the dtype trail of
// every stage is stated there.  256 threads x 8 points up to 2048 points, 1024 threads beyond (<= 8192).  Per-cloud counts and flags are
// host metadata: they are validated before anything is launched and travel as kernel arguments, BP_CHUNK clouds per launch.
#include "common.h"
#include "batchprep_body.h"

struct BpMeta { unsigned m[BP_CHUNK]; };                   // count | flags << 16 of the chunk's clouds
struct BpArgs {
    const float* raw; const int* start; const double *Rpre, *Rpost, *noise;
    float* out; int* idx;
    double sigma, clip;
    int ld, Nmax, S, ncap, b0;
};

__device__ __forceinline__ unsigned long long bp_key_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
template <int CTRL>
__device__ __forceinline__ unsigned long long bp_dpp64(unsigned long long v) {        // lanes without a source keep their own value
    const unsigned lo = __builtin_amdgcn_update_dpp((int)(unsigned)v, (int)(unsigned)v, CTRL, 0xf, 0xf, false);
    const unsigned hi = __builtin_amdgcn_update_dpp((int)(unsigned)(v >> 32), (int)(unsigned)(v >> 32), CTRL, 0xf, 0xf, false);
    return ((unsigned long long)hi << 32) | lo;
}

template <int T>
__global__ __launch_bounds__(T) void batchprep_kernel(BpArgs a, BpMeta meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bp_sm[];
    constexpr int NW = T / 64;
    const BpLds L = bp_lds(a.ncap, a.S, NW);
    float* cx = (float*)(bp_sm + L.cx);
    double* part = (double*)(bp_sm + L.part);
    double* partm = (double*)(bp_sm + L.partm);
    double* wsum = (double*)(bp_sm + L.wsum);
    double* wmax = (double*)(bp_sm + L.wmax);
    unsigned long long* slot = (unsigned long long*)(bp_sm + L.slot);
    int* sel = (int*)(bp_sm + L.sel);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = a.b0 + blockIdx.x;
    const unsigned m = meta.m[blockIdx.x];
    const int n = (int)(m & 0xffffu), fl = (int)(m >> 16), S = a.S;
    const float* xb = a.raw + (size_t)b * a.Nmax * a.ld;

    for (int j = tid; j < n; j += T) bp_stage(xb, a.ld, j, cx);
    __syncthreads();
    double c[3] = {0.0, 0.0, 0.0}, r = 1.0;
    if (!(fl & BP_F_RAW)) {                                  // (uniform over the workgroup)
        if (tid < BP_LANES) bp_sum_lane(cx, n, tid, part);
        __syncthreads();
        if (tid < BP_GROUPS) bp_sum_group(part, tid, wsum);
        __syncthreads();
        bp_centroid(wsum, n, c);
        if (tid < BP_LANES) bp_max_lane(cx, n, tid, c, partm);
        __syncthreads();
        if (tid < BP_GROUPS) bp_max_group(partm, tid, wmax);
        __syncthreads();
        r = bp_radius(wmax);
    }
    const double* R = (fl & BP_F_PRE) ? a.Rpre + (size_t)b * 9 : nullptr;
#pragma unroll 1
    for (int j = tid; j < n; j += T) bp_norm_rotate(cx, j, fl, c, r, R);     // (a thread's own points: the ones it keeps below)
    float px[BP_PPT], py[BP_PPT], pz[BP_PPT], dmin[BP_PPT];
#pragma unroll
    for (int u = 0; u < BP_PPT; ++u) {
        const int j = tid + T * u;
        // a slot past the cloud: minimum 0 for good, so its key (0, ~j) loses to every point of the cloud (lower index) -- no branch below
        px[u] = py[u] = pz[u] = 0.f; dmin[u] = j < n ? 1e10f : 0.f;
        if (j < n) { px[u] = cx[3 * j]; py[u] = cx[3 * j + 1]; pz[u] = cx[3 * j + 2]; }
    }
    __syncthreads();
    const bool sample = S < n;
    if (sample) {
        int far = bp_clamp_start(a.start[b], n);
        for (int i = 0; i < S; ++i) {
            if (tid == 0) sel[i] = far;
            const float fx = cx[3 * far], fy = cx[3 * far + 1], fz = cx[3 * far + 2];
            unsigned long long key = 0ull;
#pragma unroll
            for (int u = 0; u < BP_PPT; ++u)
                key = bp_key_max(key, bp_fps_point(px[u], py[u], pz[u], dmin[u], fx, fy, fz, tid + T * u));
            // wave max by DPP: within rows of 16 (shr 1, 2, 4, 8), then row broadcasts 15 and 31 -> lane 63 holds the wave's maximum
            key = bp_key_max(key, bp_dpp64<0x111>(key));
            key = bp_key_max(key, bp_dpp64<0x112>(key));
            key = bp_key_max(key, bp_dpp64<0x114>(key));
            key = bp_key_max(key, bp_dpp64<0x118>(key));
            key = bp_key_max(key, bp_dpp64<0x142>(key));
            key = bp_key_max(key, bp_dpp64<0x143>(key));
            if (lane == 63) slot[(i & 1) * NW + wave] = key;
            __syncthreads();
            const unsigned long long* sl = slot + (i & 1) * NW;
            unsigned long long best = sl[0];
#pragma unroll
            for (int w = 1; w < NW; ++w) best = bp_key_max(best, sl[w]);
            far = bp_key_index(best);
        }
        __syncthreads();                                     // sel is complete
    }
    const double* Q = (fl & BP_F_POST) ? a.Rpost + (size_t)b * 9 : nullptr;
    for (int i = tid; i < S; i += T) {
        const int src = sample ? sel[i] : i;
        const size_t o = (size_t)b * S + i;
        const double* nz = (fl & BP_F_JITTER) ? a.noise + o * 3 : nullptr;
        float w[3];
        bp_epilogue(cx, src, fl, Q, nz, a.sigma, a.clip, w);
        a.out[o * 3] = w[0]; a.out[o * 3 + 1] = w[1]; a.out[o * 3 + 2] = w[2];
        a.idx[o] = src;
    }
}

// counts / flags: HOST arrays (nullable: every cloud has Nmax points / no flag set).  Everything is validated before the first launch.
int launch_batch_prepare(hipStream_t st, const float* raw, int ld, int B, int Nmax, const int* counts, int S, const int* flags, const int* start,
                         const double* Rpre, const double* Rpost, const double* noise, double sigma, double clip, float* out, int* idx) {
    if (!raw || !out || !idx || B <= 0 || Nmax <= 0 || S <= 0 || ld < 3) return MLSP_ERR_ARG;
    for (int b = 0; b < B; ++b) {
        const int n = counts ? counts[b] : Nmax, fl = flags ? flags[b] : 0;
        if (n < 1 || n > Nmax || S > n || (fl & ~BP_F_ALL)) return MLSP_ERR_ARG;
        if (n > BP_MAXN) return MLSP_ERR_UNSUPPORTED;
        if (((fl & BP_F_PRE) && !Rpre) || ((fl & BP_F_POST) && !Rpost) || (S < n && !start)) return MLSP_ERR_ARG;
        if ((fl & BP_F_JITTER) && (!noise || !(clip >= 0.0) || !(sigma == sigma))) return MLSP_ERR_ARG;
    }
    for (int b0 = 0; b0 < B; b0 += BP_CHUNK) {
        const int nb = B - b0 < BP_CHUNK ? B - b0 : BP_CHUNK;
        BpMeta meta;
        int nmax = 0;
        for (int q = 0; q < nb; ++q) {
            const int n = counts ? counts[b0 + q] : Nmax, fl = flags ? flags[b0 + q] : 0;
            meta.m[q] = (unsigned)n | (unsigned)fl << 16;
            nmax = n > nmax ? n : nmax;
        }
        for (int q = nb; q < BP_CHUNK; ++q) meta.m[q] = 0u;
        BpArgs a;
        a.raw = raw; a.start = start; a.Rpre = Rpre; a.Rpost = Rpost; a.noise = noise; a.out = out; a.idx = idx;
        a.sigma = sigma; a.clip = clip; a.ld = ld; a.Nmax = Nmax; a.S = S; a.ncap = (nmax + 1) & ~1; a.b0 = b0;
        const bool wide = nmax > 256 * BP_PPT;
        const size_t lds = bp_lds(a.ncap, S, wide ? 16 : 4).bytes;
        const int rc = wide ? mlsp_launch_lds(st, batchprep_kernel<1024>, dim3(nb), dim3(1024), lds, a, meta)
                            : mlsp_launch_lds(st, batchprep_kernel<256>, dim3(nb), dim3(256), lds, a, meta);
        if (rc != MLSP_OK) return rc;
    }
    return MLSP_OK;
}
