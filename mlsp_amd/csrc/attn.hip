// What the Point-BERT transformer encoder (PointDA/model_utils.py:201-289) runs between its GEMMs: the multi-head scaled-dot-product
// attention core, LayerNorm (with the residual add and DropPath scale of the stream it normalises folded in) and GELU.  fp32 throughout.
//   mhsa fwd   one launch: a workgroup per (cloud, head, block of query rows) keeps K and V of the head in LDS; a wave owns a query row,
//              its L logits live in LDS, the softmax subtracts the row maximum; out is written head-interleaved, lse = max + log(sum).
//   mhsa bwd   one launch, a workgroup per (cloud, head), two phases: rows (K, V resident; P recomputed from lse; delta_i = sum_j P dP kept
//              in LDS; dq written) then columns (Q, dout resident; the column of P and dS recomputed; dk, dv written).  Every output
//              element has one writer: no atomics.
//   Neither direction reads or writes anything of size L^2 in global memory: the backward reads qkv, lse and dout only.
//   layernorm  a wave per row, sums across lanes through LDS in a fixed order; dgamma / dbeta as per-workgroup partials + an fp64 finaliser
//   gelu       flat, 16 bytes per thread
// The bodies are the phase functions of attn_body.h (also run on the host by tools/attn_host_check); this file owns the barriers between
// them and the launches.  Limits of the core: dh % 4 == 0, dh <= 128, L <= 512, L dh <= 16384, 16-byte-aligned rows (mhsa_geo).
#include "common.h"
#include "attn_body.h"

#define ATTN_PARTS_MAX 256

extern __shared__ __attribute__((aligned(16))) float attn_lds[];

// Traffic per (token, channel of d): 12 B of qkv read per row block that stages the head (nqb times, from L2 after the first), 4 B written.
__global__ __launch_bounds__(RT_THREADS) void mhsa_fwd_kernel(MhsaGeo g, const float* __restrict__ qkv, float* __restrict__ out,
                                                              float* __restrict__ lse) {
    const int bid = blockIdx.x, tid = threadIdx.x, d = g.H * g.dh;
    const MhsaWho o = mhsa_who(g, bid);
    mhsa_stage(g, o, tid, qkv, g.ld, d + o.h * g.dh, qkv, g.ld, 2 * d + o.h * g.dh, attn_lds);
    for (int r = 0; r < mhsa_steps(g); ++r) {
        mhsa_fwd_a(g, bid, tid, r, qkv, attn_lds);
        __syncthreads();
        mhsa_fwd_b(g, bid, tid, r, attn_lds);
        __syncthreads();
        mhsa_fwd_c(g, bid, tid, r, attn_lds);
        __syncthreads();
        mhsa_fwd_d(g, bid, tid, r, attn_lds, out, lse);
    }
}
// Traffic per (token, channel of d): 12 B of qkv and 4 B of dout read (q and dout a second time, from cache), 12 B of dqkv written.
__global__ __launch_bounds__(RT_THREADS) void mhsa_bwd_kernel(MhsaGeo g, const float* __restrict__ qkv, const float* __restrict__ lse,
                                                              const float* __restrict__ dout, float* __restrict__ dqkv) {
    const int bid = blockIdx.x, tid = threadIdx.x, d = g.H * g.dh;
    const MhsaWho o = mhsa_who(g, bid);
    mhsa_stage(g, o, tid, qkv, g.ld, d + o.h * g.dh, qkv, g.ld, 2 * d + o.h * g.dh, attn_lds);
    for (int r = 0; r < mhsa_steps(g); ++r) {
        mhsa_bwd_row_a(g, bid, tid, r, qkv, dout, attn_lds);
        __syncthreads();
        mhsa_bwd_row_b(g, bid, tid, r, lse, attn_lds);
        __syncthreads();
        mhsa_bwd_row_d(g, bid, tid, r, attn_lds, dqkv);
    }
    __syncthreads();
    mhsa_stage(g, o, tid, qkv, g.ld, o.h * g.dh, dout, d, o.h * g.dh, attn_lds);
    __syncthreads();
    mhsa_bwd_col_stats(g, bid, tid, lse, attn_lds);
    for (int r = 0; r < mhsa_steps(g); ++r) {
        mhsa_bwd_col_a(g, bid, tid, r, qkv, attn_lds);
        __syncthreads();
        mhsa_bwd_col_b(g, bid, tid, r, attn_lds);
        __syncthreads();
        mhsa_bwd_col_d(g, bid, tid, r, attn_lds, dqkv);
    }
}

// Traffic per element: x (+ a) read three times (twice from cache), u and y written: 8-16 B from memory.
__global__ __launch_bounds__(RT_THREADS) void layernorm_fwd_kernel(LnGeo g, float* __restrict__ U, float* __restrict__ Y, float* __restrict__ mean,
                                                                   float* __restrict__ rstd) {
    __shared__ float red[2 * AB_WAVES * 64];
    for (long long row0 = (long long)blockIdx.x * AB_WAVES; row0 < g.rows; row0 += (long long)gridDim.x * AB_WAVES) {
        ln_fwd_1(g, row0, threadIdx.x, U, red);
        if (!g.gamma) continue;
        __syncthreads();
        ln_fwd_2(g, row0, threadIdx.x, red);
        __syncthreads();
        ln_fwd_3(g, row0, threadIdx.x, red, Y, mean, rstd);
        __syncthreads();
    }
}
__global__ __launch_bounds__(RT_THREADS) void layernorm_bwd_kernel(LnGeo g, LnBwd b) {
    __shared__ float red[2 * AB_WAVES * 64];
    for (long long row0 = (long long)blockIdx.x * AB_WAVES; row0 < g.rows; row0 += (long long)gridDim.x * AB_WAVES) {
        ln_bwd_1(g, b, row0, threadIdx.x, red);
        __syncthreads();
        ln_bwd_2(g, b, row0, threadIdx.x, red);
        __syncthreads();
    }
}
__global__ __launch_bounds__(RT_THREADS) void layernorm_bwd_param_kernel(LnGeo g, LnBwd b, long long chunk, int ct, int rl, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sh[RT_THREADS * 8];
    const long long e0 = (long long)blockIdx.x * chunk, e1 = e0 + chunk < g.rows ? e0 + chunk : g.rows;
    for (int cq0 = 0; cq0 < g.d4; cq0 += ct) {
        ln_par_1(g, b, e0, e1, cq0, ct, rl, threadIdx.x, sh);
        __syncthreads();
        ln_par_2(g, blockIdx.x, cq0, ct, rl, threadIdx.x, sh, part);
        __syncthreads();
    }
}
__global__ __launch_bounds__(RT_THREADS) void layernorm_bwd_finalize_kernel(const float* __restrict__ part, int nparts, int d, float* __restrict__ dgamma,
                                                                            float* __restrict__ dbeta) {
    ln_par_fin(part, nparts, d, blockIdx.x * RT_THREADS + threadIdx.x, dgamma, dbeta);
}

// 8 B / 12 B per element
__global__ __launch_bounds__(RT_THREADS) void gelu_fwd_kernel(const float* __restrict__ x, long long n4, float* __restrict__ y) {
    for (long long t = (long long)blockIdx.x * RT_THREADS + threadIdx.x; t < n4; t += (long long)gridDim.x * RT_THREADS) gelu_fwd_quad(x, t, y);
}
__global__ __launch_bounds__(RT_THREADS) void gelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, long long n4,
                                                              float* __restrict__ dx) {
    for (long long t = (long long)blockIdx.x * RT_THREADS + threadIdx.x; t < n4; t += (long long)gridDim.x * RT_THREADS) gelu_bwd_quad(dy, x, t, dx);
}

// ---------------------------------------------------------------------------------------------
static inline int at_grid(long long items, int per_block, int cap) {
    const long long b = (items + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : b > cap ? cap : b);
}
static inline int mhsa_prepare(const void* kern, const MhsaGeo& g, size_t& lds) {
    lds = mhsa_lds_floats(g) * sizeof(float);
    if (lds > 64 * 1024) {
        hipError_t e = mlsp_lds_limit(kern, lds);
        if (e != hipSuccess) return (int)e;
    }
    return MLSP_OK;
}
int launch_mhsa_fwd(hipStream_t st, const float* qkv, int ld, int B, int L, int H, int dh, float scale, float* out, float* lse) {
    MhsaGeo g;
    if (!mhsa_geo(B, L, H, dh, ld, ld, scale, false, g) || !al16(qkv, out)) return MLSP_ERR_UNSUPPORTED;
    size_t lds;
    const int rc = mhsa_prepare((const void*)mhsa_fwd_kernel, g, lds);
    if (rc != MLSP_OK) return rc;
    hipLaunchKernelGGL(mhsa_fwd_kernel, dim3(B * H * g.nqb), dim3(RT_THREADS), lds, st, g, qkv, out, lse);
    return mlsp_launch_status();
}
int launch_mhsa_bwd(hipStream_t st, const float* qkv, int ld, const float* lse, const float* dout, int B, int L, int H, int dh, float scale,
                    float* dqkv, int ldd) {
    MhsaGeo g;
    if (!mhsa_geo(B, L, H, dh, ld, ldd, scale, true, g) || !al16(qkv, dout, dqkv)) return MLSP_ERR_UNSUPPORTED;
    size_t lds;
    const int rc = mhsa_prepare((const void*)mhsa_bwd_kernel, g, lds);
    if (rc != MLSP_OK) return rc;
    hipLaunchKernelGGL(mhsa_bwd_kernel, dim3(B * H * g.nqb), dim3(RT_THREADS), lds, st, g, qkv, lse, dout, dqkv);
    return mlsp_launch_status();
}

static inline bool ln_shape_ok(long long rows, int d, const float* s, int rps) {
    return rows > 0 && rows <= (1LL << 40) && d > 0 && d % 4 == 0 && d <= (1 << 20) && (!s || rps > 0);
}
int launch_layernorm_fwd(hipStream_t st, const float* x, const float* a, const float* s, int rows_per_sample, const float* gamma, const float* beta,
                         long long rows, int d, float eps, float* u, float* y, float* mean, float* rstd) {
    if (!ln_shape_ok(rows, d, s, rows_per_sample) || !al16(x, a, gamma, beta, u, y))
        return MLSP_ERR_UNSUPPORTED;
    const LnGeo g{rows, d / 4, rows_per_sample, eps, x, a, s, gamma, beta};
    hipLaunchKernelGGL(layernorm_fwd_kernel, dim3(at_grid(rows, AB_WAVES, 1 << 16)), dim3(RT_THREADS), 0, st, g, u, y, mean, rstd);
    return mlsp_launch_status();
}
// the split of the rows among the workgroups of the dgamma / dbeta pass: (channel threads, row lanes, workgroups)
static inline void ln_par_plan(long long rows, int d, int& ct, int& rl, int& nparts) {
    const int d4 = d / 4;
    ct = d4 < RT_THREADS ? d4 : RT_THREADS;
    rl = RT_THREADS / ct;
    const long long want = (rows + (long long)rl * 8 - 1) / ((long long)rl * 8);
    nparts = (int)(want < 1 ? 1 : want > ATTN_PARTS_MAX ? ATTN_PARTS_MAX : want);
}
size_t layernorm_bwd_ws_floats(long long rows, int d) {
    int ct, rl, nparts;
    ln_par_plan(rows, d, ct, rl, nparts);
    return (size_t)nparts * d * 2;
}
int launch_layernorm_bwd(hipStream_t st, const float* dy, const float* du, const float* u, const float* s, int rows_per_sample, const float* gamma,
                         const float* mean, const float* rstd, long long rows, int d, float* dx, float* da, float* part, float* dgamma,
                         float* dbeta) {
    if (!ln_shape_ok(rows, d, s, rows_per_sample) || !al16(dy, du, u, gamma, dx, da, part))
        return MLSP_ERR_UNSUPPORTED;
    const LnGeo g{rows, d / 4, rows_per_sample, 0.f, u, nullptr, s, gamma, nullptr};
    const LnBwd b{dy, du, mean, rstd, dx, da};
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3(at_grid(rows, AB_WAVES, 1 << 16)), dim3(RT_THREADS), 0, st, g, b);
    if (dy) {
        int ct, rl, nparts;
        ln_par_plan(rows, d, ct, rl, nparts);
        const long long chunk = (rows + nparts - 1) / nparts;
        hipLaunchKernelGGL(layernorm_bwd_param_kernel, dim3(nparts), dim3(RT_THREADS), 0, st, g, b, chunk, ct, rl, part);
        hipLaunchKernelGGL(layernorm_bwd_finalize_kernel, dim3((d + RT_THREADS - 1) / RT_THREADS), dim3(RT_THREADS), 0, st, part, nparts, d, dgamma,
                           dbeta);
    }
    return mlsp_launch_status();
}
int launch_gelu_fwd(hipStream_t st, const float* x, long long rows, int d, float* y) {
    if (rows <= 0 || d <= 0 || d % 4 || !al16(x, y)) return MLSP_ERR_UNSUPPORTED;
    const long long n4 = rows * (d / 4);
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3(at_grid(n4, RT_THREADS, 65536)), dim3(RT_THREADS), 0, st, x, n4, y);
    return mlsp_launch_status();
}
int launch_gelu_bwd(hipStream_t st, const float* dy, const float* x, long long rows, int d, float* dx) {
    if (rows <= 0 || d <= 0 || d % 4 || !al16(dy, x, dx)) return MLSP_ERR_UNSUPPORTED;
    const long long n4 = rows * (d / 4);
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3(at_grid(n4, RT_THREADS, 65536)), dim3(RT_THREADS), 0, st, dy, x, n4, dx);
    return mlsp_launch_status();
}
