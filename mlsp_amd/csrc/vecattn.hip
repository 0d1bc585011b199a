// The edge stages of the Hengshuang Point Transformer block (PointDA/hengshuang_transformer/transformer.py:28-44) between its GEMMs:
//   delta      :37      H1[e] = relu(Wd1 (xyz_i - xyz_j) + bd1)               first layer of fc_delta (K = 3: arithmetic, not a GEMM)
//   mix        :39      T[e]  = q_i - kk_j + pos[e]                            the input of fc_gamma
//   aggregate  :40-42   attn  = softmax_s(A / sqrt(d)),  res_i = sum_s attn[i,s] * (v_j + pos[i,s])
//   relu                the ReLU between the two layers of fc_gamma (the GEMM family activates only behind a BatchNorm)
// e = (i, s) is slot s of point i (P = B N points, k slots each, E = P k edges), j = idx[i][s] its neighbour, local to the cloud.  Every
// [E][d] / [P][d] matrix is fp32 with the channels contiguous; a thread owns 4 channels (one 16-byte access) of one edge (delta, mix, relu)
// or of one point, walking its k slots (aggregate, mix_bwd).  Element offsets are 64-bit (E d exceeds 2^31 at the model's sizes).  No
// atomics: the sums over slots run in ascending s in one thread, delta_bwd's sums over edges in a fixed order (per-workgroup partials in
// the workspace + a finalising pass); the scatters back to the neighbours (dkk_j, dv_j) go through the reverse index of sa.hip.
// All kernels stream HBM once or twice; bytes per edge and channel are listed at each kernel.
// Bounds: d % 4 == 0, 1 <= k <= VA_MAX_K, 16-byte-aligned pointers and row pitches.  An index outside [0, N) is read as 0 (never
// dereferenced out of the cloud).
#include "common.h"
#include "rowtile.h"
#include <math.h>

#define VA_MAX_K 64
#define VA_PARTS_MAX 1024

__device__ __forceinline__ int va_nbr(const int* __restrict__ idx, long long e, int N) {
    const int j = idx[e];
    return (unsigned)j < (unsigned)N ? j : 0;
}

// ---------------------------------------------------------------------------------------------
// H1[e][c] = relu(((r0 W[c][0] + r1 W[c][1]) + r2 W[c][2]) + b[c]) as an fma chain, r = xyz_i - xyz_j subtracted first (:37).
// Traffic per edge and channel: 4 B written (the coordinates and the 16 d bytes of weights stay in cache).
__global__ __launch_bounds__(RT_THREADS) void vecattn_delta_fwd_kernel(const float* __restrict__ xyz, int ldx, const int* __restrict__ idx,
                                                                       const float* __restrict__ Wd1, const float* __restrict__ bd1, int N,
                                                                       int k, int d4, long long E, int rb, float* __restrict__ H1) {
    RT_FOR_ITEMS(E, rb, d4, RT_THREADS) {
        const int lr = it_ / d4, cq = it_ - lr * d4;
        const long long e = r0_ + lr, i = e / k, cloud = i / N;
        const long long j = cloud * N + va_nbr(idx, e, N);
        const float* pi = xyz + i * ldx;
        const float* pj = xyz + j * ldx;
        const float r0 = pi[0] - pj[0], r1 = pi[1] - pj[1], r2 = pi[2] - pj[2];
        const float* w = Wd1 + (size_t)cq * 12;         // rows 4 cq .. 4 cq + 3 of [d][3]: 12 contiguous floats
        const f32x4 w0 = rt_ld(w), w1 = rt_ld(w + 4), w2 = rt_ld(w + 8), b = rt_ld(bd1 + cq * 4);
        f32x4 h;
        h.x = fmaf(r2, w0.z, fmaf(r1, w0.y, r0 * w0.x)) + b.x;
        h.y = fmaf(r2, w1.y, fmaf(r1, w1.x, r0 * w0.w)) + b.y;
        h.z = fmaf(r2, w2.x, fmaf(r1, w1.w, r0 * w1.z)) + b.z;
        h.w = fmaf(r2, w2.w, fmaf(r1, w2.z, r0 * w2.y)) + b.w;
        h.x = fmaxf(h.x, 0.f); h.y = fmaxf(h.y, 0.f); h.z = fmaxf(h.z, 0.f); h.w = fmaxf(h.w, 0.f);
        rt_st(H1 + (e * d4 + cq) * 4, h);
    }
}

// dWd1[c][a] = sum_e m r_a, dbd1[c] = sum_e m, m = dH1[e][c] where H1[e][c] > 0.  Workgroup g sums the edges [g chunk, (g + 1) chunk):
// its threads are (row lane, channel quad), a thread keeps 4 channels x {r0, r1, r2, 1} in registers over every rl-th edge, the row lanes
// are summed through LDS in ascending lane order and part[g][c] = {dW[c][0..2], db[c]} is written; the finalising pass sums the parts in
// ascending g in fp64.  Traffic per edge and channel: 8 B read.
__global__ __launch_bounds__(RT_THREADS) void vecattn_delta_bwd_kernel(const float* __restrict__ dH1, const float* __restrict__ H1,
                                                                       const float* __restrict__ xyz, int ldx, const int* __restrict__ idx,
                                                                       int N, int k, int d4, long long E, long long chunk, int ct, int rl,
                                                                       f32x4* __restrict__ part) {
    __shared__ f32x4 sh[RT_THREADS * 4];
    const int tid = threadIdx.x, tc = tid % ct, r = tid / ct;
    const long long e0 = (long long)blockIdx.x * chunk, e1 = e0 + chunk < E ? e0 + chunk : E;
    for (int cq0 = 0; cq0 < d4; cq0 += ct) {
        const int cq = cq0 + tc;
        const bool live = r < rl && cq < d4;
        f32x4 acc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (live)
            for (long long e = e0 + r; e < e1; e += rl) {
                const long long i = e / k, cloud = i / N;
                const long long j = cloud * N + va_nbr(idx, e, N);
                const float* pi = xyz + i * ldx;
                const float* pj = xyz + j * ldx;
                const float r0 = pi[0] - pj[0], r1 = pi[1] - pj[1], r2 = pi[2] - pj[2];
                const f32x4 g = rt_ld(dH1 + (e * d4 + cq) * 4), h = rt_ld(H1 + (e * d4 + cq) * 4);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float m = h[u] > 0.f ? g[u] : 0.f;
                    acc[u].x += m * r0; acc[u].y += m * r1; acc[u].z += m * r2; acc[u].w += m;
                }
            }
#pragma unroll
        for (int u = 0; u < 4; ++u) sh[tid * 4 + u] = acc[u];
        __syncthreads();
        if (live && r == 0) {
            for (int q = 1; q < rl; ++q)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[u] += sh[(q * ct + tc) * 4 + u];
#pragma unroll
            for (int u = 0; u < 4; ++u) part[((size_t)blockIdx.x * d4 + cq) * 4 + u] = acc[u];
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(RT_THREADS) void vecattn_delta_bwd_finalize_kernel(const f32x4* __restrict__ part, int nparts, int d,
                                                                                float* __restrict__ dWd1, float* __restrict__ dbd1) {
    const int c = blockIdx.x * RT_THREADS + threadIdx.x;
    if (c >= d) return;
    double x = 0.0, y = 0.0, z = 0.0, w = 0.0;
    for (int g = 0; g < nparts; ++g) {
        const f32x4 p = part[(size_t)g * d + c];
        x += p.x; y += p.y; z += p.z; w += p.w;
    }
    dWd1[c * 3] = (float)x; dWd1[c * 3 + 1] = (float)y; dWd1[c * 3 + 2] = (float)z;
    dbd1[c] = (float)w;
}

// ---------------------------------------------------------------------------------------------
// T[e] = (q_i - kk_j) + pos[e] (:39).  Traffic per edge and channel: 4 B read (pos) + 4 B written; the q / kk rows come from cache.
__global__ __launch_bounds__(RT_THREADS) void vecattn_mix_fwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kk, int ldk,
                                                                     const float* __restrict__ pos, const int* __restrict__ idx, int N, int k,
                                                                     int d4, long long E, int rb, float* __restrict__ T) {
    RT_FOR_ITEMS(E, rb, d4, RT_THREADS) {
        const int lr = it_ / d4, cq = it_ - lr * d4;
        const long long e = r0_ + lr, i = e / k, cloud = i / N;
        const long long j = cloud * N + va_nbr(idx, e, N);
        const f32x4 a = rt_ld(q + i * ldq + cq * 4), b = rt_ld(kk + j * ldk + cq * 4), p = rt_ld(pos + (e * d4 + cq) * 4);
        rt_st(T + (e * d4 + cq) * 4, (a - b) + p);
    }
}
// dq_i = sum_s dT[i][s] in ascending s.  Traffic per edge and channel: 4 B read.
__global__ __launch_bounds__(RT_THREADS) void vecattn_mix_bwd_kernel(const float* __restrict__ dT, int k, int d4, long long P, int rb,
                                                                     float* __restrict__ dq) {
    RT_FOR_ITEMS(P, rb, d4, RT_THREADS) {
        const int lr = it_ / d4, cq = it_ - lr * d4;
        const long long i = r0_ + lr;
        const float* g = dT + (i * k * d4 + cq) * 4;
        f32x4 s = rt_ld(g);
        for (int u = 1; u < k; ++u) s += rt_ld(g + (size_t)u * d4 * 4);
        rt_st(dq + (i * d4 + cq) * 4, s);
    }
}

// ---------------------------------------------------------------------------------------------
// Softmax over the k slots of a point per channel, of A / sqrt(d), and the weighted sum (:40-42).  First walk: running maximum and the
// sum of exp(x - max) rescaled whenever the maximum moves (registers only); second walk: attn = exp(x - max) / sum, written, and
// res += attn * (v_j + pos).  Traffic per edge and channel: 4 B (A) + 4 B (pos) read, 4 B (attn) written; A's second read comes
// from L2 (a tile's k rows were just read), the v rows from cache.
__global__ __launch_bounds__(RT_THREADS) void vecattn_aggregate_fwd_kernel(const float* __restrict__ A, const float* __restrict__ v, int ldv,
                                                                           const float* __restrict__ pos, const int* __restrict__ idx, int N,
                                                                           int k, int d4, long long P, int rb, float sq,
                                                                           float* __restrict__ attn, float* __restrict__ res) {
    RT_FOR_ITEMS(P, rb, d4, RT_THREADS) {
        const int lr = it_ / d4, cq = it_ - lr * d4;
        const long long i = r0_ + lr, cloud = i / N, e0 = i * k;
        const float* a = A + (e0 * d4 + cq) * 4;
        f32x4 m = rt_ld(a) / sq, l = f32x4{1.f, 1.f, 1.f, 1.f};
        for (int s = 1; s < k; ++s) {
            const f32x4 x = rt_ld(a + (size_t)s * d4 * 4) / sq;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float mn = fmaxf(m[u], x[u]);
                l[u] = l[u] * expf(m[u] - mn) + expf(x[u] - mn);
                m[u] = mn;
            }
        }
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < k; ++s) {
            const long long e = e0 + s, j = cloud * N + va_nbr(idx, e, N);
            const f32x4 x = rt_ld(a + (size_t)s * d4 * 4) / sq;
            const f32x4 vp = rt_ld(v + j * ldv + cq * 4) + rt_ld(pos + (e * d4 + cq) * 4);
            f32x4 w;
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = expf(x[u] - m[u]) / l[u];
            rt_st(attn + (e * d4 + cq) * 4, w);
            acc += w * vp;
        }
        rt_st(res + (i * d4 + cq) * 4, acc);
    }
}
// dVP[e] = attn[e] * dres_i;  dA[e] = attn[e] * (g[e] - sum_s attn[i,s] g[i,s]) / sqrt(d),  g[e] = dres_i * (v_j + pos[e]).
// First walk: dVP and the sum; second walk: dA.  Traffic per edge and channel: 8 B read (attn, pos) + 8 B written; the second reads
// of attn and pos come from L2.
__global__ __launch_bounds__(RT_THREADS) void vecattn_aggregate_bwd_kernel(const float* __restrict__ dres, const float* __restrict__ attn,
                                                                           const float* __restrict__ v, int ldv, const float* __restrict__ pos,
                                                                           const int* __restrict__ idx, int N, int k, int d4, long long P, int rb,
                                                                           float sq, float* __restrict__ dVP, float* __restrict__ dA) {
    RT_FOR_ITEMS(P, rb, d4, RT_THREADS) {
        const int lr = it_ / d4, cq = it_ - lr * d4;
        const long long i = r0_ + lr, cloud = i / N, e0 = i * k;
        const f32x4 dr = rt_ld(dres + (i * d4 + cq) * 4);
        f32x4 dot = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < k; ++s) {
            const long long e = e0 + s, j = cloud * N + va_nbr(idx, e, N);
            const f32x4 w = rt_ld(attn + (e * d4 + cq) * 4);
            const f32x4 vp = rt_ld(v + j * ldv + cq * 4) + rt_ld(pos + (e * d4 + cq) * 4);
            rt_st(dVP + (e * d4 + cq) * 4, w * dr);
            dot += w * (dr * vp);
        }
        for (int s = 0; s < k; ++s) {
            const long long e = e0 + s, j = cloud * N + va_nbr(idx, e, N);
            const f32x4 w = rt_ld(attn + (e * d4 + cq) * 4);
            const f32x4 vp = rt_ld(v + j * ldv + cq * 4) + rt_ld(pos + (e * d4 + cq) * 4);
            rt_st(dA + (e * d4 + cq) * 4, w * (dr * vp - dot) / sq);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// y = max(x, 0) (y may be x);  dx = dy where y > 0, else 0.  n4 quads.  8 B / 12 B per element.
__global__ __launch_bounds__(RT_THREADS) void vecattn_relu_fwd_kernel(const float* __restrict__ x, long long n4, float* __restrict__ y) {
    for (long long t = (long long)blockIdx.x * RT_THREADS + threadIdx.x; t < n4; t += (long long)gridDim.x * RT_THREADS) {
        f32x4 a = rt_ld(x + t * 4);
        a.x = fmaxf(a.x, 0.f); a.y = fmaxf(a.y, 0.f); a.z = fmaxf(a.z, 0.f); a.w = fmaxf(a.w, 0.f);
        rt_st(y + t * 4, a);
    }
}
__global__ __launch_bounds__(RT_THREADS) void vecattn_relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, long long n4,
                                                                      float* __restrict__ dx) {
    for (long long t = (long long)blockIdx.x * RT_THREADS + threadIdx.x; t < n4; t += (long long)gridDim.x * RT_THREADS) {
        const f32x4 g = rt_ld(dy + t * 4), a = rt_ld(y + t * 4);
        rt_st(dx + t * 4, f32x4{a.x > 0.f ? g.x : 0.f, a.y > 0.f ? g.y : 0.f, a.z > 0.f ? g.z : 0.f, a.w > 0.f ? g.w : 0.f});
    }
}

// ---------------------------------------------------------------------------------------------
static inline bool va_shape_ok(int B, int N, int k, int d) {
    return d % 4 == 0 && k >= 1 && k <= VA_MAX_K && (long long)B * N <= (1LL << 30);
}
// delta_bwd's split of the E edges: (channel threads, row lanes, workgroups)
static inline void va_delta_bwd_plan(long long E, int d, int& ct, int& rl, int& nparts) {
    const int d4 = d / 4;
    ct = d4 < RT_THREADS ? d4 : RT_THREADS;
    rl = RT_THREADS / ct;
    const long long want = (E + (long long)rl * 8 - 1) / ((long long)rl * 8);
    nparts = (int)(want < 1 ? 1 : want > VA_PARTS_MAX ? VA_PARTS_MAX : want);
}
size_t vecattn_delta_bwd_ws_floats(int B, int N, int k, int d) {
    int ct, rl, nparts;
    va_delta_bwd_plan((long long)B * N * k, d, ct, rl, nparts);
    return (size_t)nparts * d * 4;
}

int launch_vecattn_delta_fwd(hipStream_t st, const float* xyz, int ldx, const int* idx, const float* Wd1, const float* bd1, int B, int N, int k,
                             int d, float* H1) {
    if (!va_shape_ok(B, N, k, d) || ldx < 3 || !al16(Wd1, bd1, H1)) return MLSP_ERR_UNSUPPORTED;
    const long long E = (long long)B * N * k;
    const RowTiles t = row_tiles(E, d / 4);
    hipLaunchKernelGGL(vecattn_delta_fwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, xyz, ldx, idx, Wd1, bd1, N, k, d / 4, E, t.rb, H1);
    return mlsp_launch_status();
}
int launch_vecattn_delta_bwd(hipStream_t st, const float* dH1, const float* H1, const float* xyz, int ldx, const int* idx, int B, int N, int k,
                             int d, float* part, float* dWd1, float* dbd1) {
    if (!va_shape_ok(B, N, k, d) || ldx < 3 || !al16(dH1, H1, part)) return MLSP_ERR_UNSUPPORTED;
    const long long E = (long long)B * N * k;
    int ct, rl, nparts;
    va_delta_bwd_plan(E, d, ct, rl, nparts);
    const long long chunk = (E + nparts - 1) / nparts;
    hipLaunchKernelGGL(vecattn_delta_bwd_kernel, dim3(nparts), dim3(RT_THREADS), 0, st, dH1, H1, xyz, ldx, idx, N, k, d / 4, E, chunk, ct, rl,
                       (f32x4*)part);
    hipLaunchKernelGGL(vecattn_delta_bwd_finalize_kernel, dim3((d + RT_THREADS - 1) / RT_THREADS), dim3(RT_THREADS), 0, st,
                       (const f32x4*)part, nparts, d, dWd1, dbd1);
    return mlsp_launch_status();
}
int launch_vecattn_mix_fwd(hipStream_t st, const float* q, int ldq, const float* kk, int ldk, const float* pos, const int* idx, int B, int N, int k,
                           int d, float* T) {
    if (!va_shape_ok(B, N, k, d) || ldq < d || ldk < d || ldq % 4 || ldk % 4 || !al16(q, kk, pos, T))
        return MLSP_ERR_UNSUPPORTED;
    const long long E = (long long)B * N * k;
    const RowTiles t = row_tiles(E, d / 4);
    hipLaunchKernelGGL(vecattn_mix_fwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, q, ldq, kk, ldk, pos, idx, N, k, d / 4, E, t.rb, T);
    return mlsp_launch_status();
}
int launch_vecattn_mix_bwd(hipStream_t st, const float* dT, int B, int N, int k, int d, float* dq) {
    if (!va_shape_ok(B, N, k, d) || !al16(dT, dq)) return MLSP_ERR_UNSUPPORTED;
    const long long P = (long long)B * N;
    const RowTiles t = row_tiles(P, d / 4);
    hipLaunchKernelGGL(vecattn_mix_bwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, dT, k, d / 4, P, t.rb, dq);
    return mlsp_launch_status();
}
int launch_vecattn_aggregate_fwd(hipStream_t st, const float* A, const float* v, int ldv, const float* pos, const int* idx, int B, int N, int k,
                                 int d, float* attn, float* res) {
    if (!va_shape_ok(B, N, k, d) || ldv < d || ldv % 4 || !al16(A, v, pos, attn, res))
        return MLSP_ERR_UNSUPPORTED;
    const long long P = (long long)B * N;
    const RowTiles t = row_tiles(P, d / 4);
    hipLaunchKernelGGL(vecattn_aggregate_fwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, A, v, ldv, pos, idx, N, k, d / 4, P, t.rb,
                       sqrtf((float)d), attn, res);
    return mlsp_launch_status();
}
int launch_vecattn_aggregate_bwd(hipStream_t st, const float* dres, const float* attn, const float* v, int ldv, const float* pos, const int* idx,
                                 int B, int N, int k, int d, float* dVP, float* dA) {
    if (!va_shape_ok(B, N, k, d) || ldv < d || ldv % 4 || !al16(dres, attn, v, pos, dVP, dA))
        return MLSP_ERR_UNSUPPORTED;
    const long long P = (long long)B * N;
    const RowTiles t = row_tiles(P, d / 4);
    hipLaunchKernelGGL(vecattn_aggregate_bwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, dres, attn, v, ldv, pos, idx, N, k, d / 4, P, t.rb,
                       sqrtf((float)d), dVP, dA);
    return mlsp_launch_status();
}
static inline int va_flat_grid(long long n4) {
    const long long b = (n4 + RT_THREADS - 1) / RT_THREADS;
    return (int)(b < 1 ? 1 : b > 65536 ? 65536 : b);
}
int launch_vecattn_relu_fwd(hipStream_t st, const float* x, long long rows, int d, float* y) {
    if (rows <= 0 || d <= 0 || d % 4 || !al16(x, y)) return MLSP_ERR_UNSUPPORTED;
    const long long n4 = rows * (d / 4);
    hipLaunchKernelGGL(vecattn_relu_fwd_kernel, dim3(va_flat_grid(n4)), dim3(RT_THREADS), 0, st, x, n4, y);
    return mlsp_launch_status();
}
int launch_vecattn_relu_bwd(hipStream_t st, const float* dy, const float* y, long long rows, int d, float* dx) {
    if (rows <= 0 || d <= 0 || d % 4 || !al16(dy, y, dx)) return MLSP_ERR_UNSUPPORTED;
    const long long n4 = rows * (d / 4);
    hipLaunchKernelGGL(vecattn_relu_bwd_kernel, dim3(va_flat_grid(n4)), dim3(RT_THREADS), 0, st, dy, y, n4, dx);
    return mlsp_launch_status();
}
