// The edge stage of DGCNN_Propagation (PointDA/Models.py:327-363) behind its folded convolution: with the conv weight W = [Wa | Wb] over
// the edge input [f_j - f_i ; f_i], the pre-norm value of edge (i, s) is y = u_j + w_i, u = f_k Wa^T per source point, w = f_q (Wb - Wa)^T
// per query point (two per-point GEMMs the caller runs), j = idx[i][s] local to the cloud.  These kernels do what follows the conv --
// GroupNorm over (cloud, channel group), LeakyReLU, max over the k slots (:356-357, :360-361) -- and its backward, without the [E][C] edge
// tensor in either direction (E = B Nq k).  The bodies are the phase functions of gnedge_body.h (tools/gn_edge_host_check runs them on the host).
//   stats      sums of y, y^2 per (cloud, group): fp64 per-workgroup partials in the workspace + a finaliser in ascending order
//   apply      out = lrelu(GroupNorm(y at the selected slot)), argk: the maximum of y where gamma rstd >= 0, the minimum otherwise
//   bsum       per-channel sums of dz yhat_sel and dz over the selected entries: fp32 partials + fp64 finalisers (dgamma, dbeta, and the
//              group means A, Bm of GroupNorm's backward)
//   dw, du     dy = rstd (gamma dz [s == argk] - A - yhat Bm) summed over a query's slots (ascending s) / over the edges that name a source
//              point (reverse-index order)
// fp32, channels contiguous, a thread owns 4 channels, 64-bit element offsets, no atomics, every sum in a fixed order.
// Traffic per edge and channel (u / w rows come from cache: a cloud's u is Nk C floats): stats 4 B of u gathered; apply 4 B gathered +
// (4 + 1) / k B written; bsum (4 + 4 + 1) / k B; dw 4 B gathered + 4 / k B written; du 4 B (w) + 4 B (dOut) + 1 B (argk) gathered.
// Bounds: C % (4 groups) == 0, 1 <= k <= 64, groups <= 256, 16-byte-aligned pointers and row pitches.
#include "common.h"
#include "gnedge_body.h"

// workgroup (p, b) = blockIdx.x % np, blockIdx.x / np
__global__ __launch_bounds__(RT_THREADS) void gn_edge_stats_kernel(GeGeo g, double* __restrict__ part) {
    __shared__ double sh[RT_THREADS * 2];
    const int b = blockIdx.x / g.np, p = blockIdx.x - b * g.np;
    for (int cq0 = 0; cq0 < g.c4; cq0 += g.ct) {
        ge_stats_1(g, b, p, cq0, threadIdx.x, sh);
        __syncthreads();
        ge_stats_2(g, b, p, cq0, threadIdx.x, sh, part);
        __syncthreads();
    }
}
__global__ __launch_bounds__(RT_THREADS) void gn_edge_stats_finalize_kernel(GeGeo g, const double* __restrict__ part, float* __restrict__ stats) {
    ge_stats_fin(g, (long long)blockIdx.x * RT_THREADS + threadIdx.x, part, stats);
}
__global__ __launch_bounds__(RT_THREADS) void gn_edge_apply_kernel(GeGeo g, int rb, const float* __restrict__ stats, float* __restrict__ out,
                                                                   uint8_t* __restrict__ argk) {
    const long long P = (long long)g.B * g.Nq;
    RT_FOR_ITEMS(P, rb, g.c4, RT_THREADS) {
        const int lr = it_ / g.c4;
        ge_apply_item(g, r0_ + lr, it_ - lr * g.c4, stats, out, argk);
    }
}

__global__ __launch_bounds__(RT_THREADS) void gn_edge_bsum_kernel(GeGeo g, const float* __restrict__ stats, const float* __restrict__ dOut,
                                                                  const uint8_t* __restrict__ argk, float* __restrict__ chpart) {
    __shared__ __attribute__((aligned(16))) float sh[RT_THREADS * 8];
    const int b = blockIdx.x / g.np, p = blockIdx.x - b * g.np;
    for (int cq0 = 0; cq0 < g.c4; cq0 += g.ct) {
        ge_bsum_1(g, b, p, cq0, threadIdx.x, stats, dOut, argk, sh);
        __syncthreads();
        ge_bsum_2(g, b, p, cq0, threadIdx.x, sh, chpart);
        __syncthreads();
    }
}
// a workgroup per cloud; `cloud` is written in phase 1 and read in phase 2 by other threads of the same workgroup
__global__ __launch_bounds__(RT_THREADS) void gn_edge_bfin_cloud_kernel(GeGeo g, const float* __restrict__ chpart, double* cloud, float* __restrict__ ab) {
    ge_bfin_1(g, blockIdx.x, threadIdx.x, chpart, cloud);
    __threadfence_block();
    __syncthreads();
    ge_bfin_2(g, blockIdx.x, threadIdx.x, cloud, ab);
}
__global__ __launch_bounds__(RT_THREADS) void gn_edge_bfin_param_kernel(GeGeo g, const double* __restrict__ cloud, float* __restrict__ dgamma,
                                                                        float* __restrict__ dbeta) {
    ge_bfin_param(g, blockIdx.x * RT_THREADS + threadIdx.x, cloud, dgamma, dbeta);
}
__global__ __launch_bounds__(RT_THREADS) void gn_edge_bwd_dw_kernel(GeGeo g, int rb, const float* __restrict__ stats, const float* __restrict__ ab,
                                                                    const float* __restrict__ dOut, const uint8_t* __restrict__ argk,
                                                                    float* __restrict__ dw) {
    const long long P = (long long)g.B * g.Nq;
    RT_FOR_ITEMS(P, rb, g.c4, RT_THREADS) {
        const int lr = it_ / g.c4;
        ge_bwd_dw_item(g, r0_ + lr, it_ - lr * g.c4, stats, ab, dOut, argk, dw);
    }
}
__global__ __launch_bounds__(RT_THREADS) void gn_edge_bwd_du_kernel(GeGeo g, int rb, const float* __restrict__ stats, const float* __restrict__ ab,
                                                                    const float* __restrict__ dOut, const uint8_t* __restrict__ argk,
                                                                    const int* __restrict__ rev_off, const int* __restrict__ rev_ent,
                                                                    float* __restrict__ du) {
    const long long P = (long long)g.B * g.Nk;
    RT_FOR_ITEMS(P, rb, g.c4, RT_THREADS) {
        const int lr = it_ / g.c4;
        ge_bwd_du_item(g, r0_ + lr, it_ - lr * g.c4, stats, ab, dOut, argk, rev_off, rev_ent, du);
    }
}

// ---------------------------------------------------------------------------------------------
static inline bool ge_setup(const float* u, int ldu, const float* w, int ldw, const int* idx, const float* gamma, const float* beta, int B, int Nk,
                            int Nq, int k, int C, int groups, float eps, float slope, GeGeo& g) {
    if (!ge_geo(B, Nk, Nq, k, C, groups, ldu, ldw, eps, slope, g) || !al16(u, w, gamma, beta)) return false;
    g.u = u; g.w = w; g.idx = idx; g.gamma = gamma; g.beta = beta;
    return true;
}
size_t gn_edge_ws_bytes(int B, int Nk, int Nq, int k, int C, int groups) {
    GeGeo g;
    if (!ge_geo(B, Nk, Nq, k, C, groups, C, C, 0.f, 0.f, g)) return 0;
    const size_t fwd = align_up(ge_fwd_ws_doubles(g) * sizeof(double), 256);
    const size_t bwd = align_up(ge_bwd_ws_floats(g) * sizeof(float), 256) + align_up(ge_bwd_ws_doubles(g) * sizeof(double), 256) +
                       align_up((size_t)B * groups * 2 * sizeof(float), 256);
    return (fwd > bwd ? fwd : bwd) + MLSP_AMAX_TAIL_BYTES;
}
int launch_gn_edge_fwd(hipStream_t st, const float* u, int ldu, const float* w, int ldw, const int* idx, const float* gamma, const float* beta,
                       int B, int Nk, int Nq, int k, int C, int groups, float eps, float slope, float* out, uint8_t* argk, float* stats,
                       Workspace& ws) {
    GeGeo g;
    if (!ge_setup(u, ldu, w, ldw, idx, gamma, beta, B, Nk, Nq, k, C, groups, eps, slope, g) || !al16(out)) return MLSP_ERR_UNSUPPORTED;
    double* part = ws.take<double>(ge_fwd_ws_doubles(g));
    if (!ws.ok()) return MLSP_ERR_WORKSPACE;
    const RowTiles t = row_tiles((long long)B * Nq, g.c4);
    hipLaunchKernelGGL(gn_edge_stats_kernel, dim3(B * g.np), dim3(RT_THREADS), 0, st, g, part);
    hipLaunchKernelGGL(gn_edge_stats_finalize_kernel, dim3((B * groups + RT_THREADS - 1) / RT_THREADS), dim3(RT_THREADS), 0, st, g, part, stats);
    hipLaunchKernelGGL(gn_edge_apply_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, g, t.rb, stats, out, argk);
    return mlsp_launch_status();
}
int launch_gn_edge_bwd(hipStream_t st, const float* dOut, const float* u, int ldu, const float* w, int ldw, const int* idx, const uint8_t* argk,
                       const float* stats, const int* rev_off, const int* rev_ent, const float* gamma, const float* beta, int B, int Nk, int Nq,
                       int k, int C, int groups, float slope, float* du, float* dw, float* dgamma, float* dbeta, Workspace& ws) {
    GeGeo g;
    if (!ge_setup(u, ldu, w, ldw, idx, gamma, beta, B, Nk, Nq, k, C, groups, 0.f, slope, g) || !al16(dOut, du, dw))
        return MLSP_ERR_UNSUPPORTED;
    float* chpart = ws.take<float>(ge_bwd_ws_floats(g));
    double* cloud = ws.take<double>(ge_bwd_ws_doubles(g));
    float* ab = ws.take<float>((size_t)B * groups * 2);
    if (!ws.ok()) return MLSP_ERR_WORKSPACE;
    hipLaunchKernelGGL(gn_edge_bsum_kernel, dim3(B * g.np), dim3(RT_THREADS), 0, st, g, stats, dOut, argk, chpart);
    hipLaunchKernelGGL(gn_edge_bfin_cloud_kernel, dim3(B), dim3(RT_THREADS), 0, st, g, chpart, cloud, ab);
    hipLaunchKernelGGL(gn_edge_bfin_param_kernel, dim3((C + RT_THREADS - 1) / RT_THREADS), dim3(RT_THREADS), 0, st, g, cloud, dgamma, dbeta);
    const RowTiles tq = row_tiles((long long)B * Nq, g.c4), tk = row_tiles((long long)B * Nk, g.c4);
    hipLaunchKernelGGL(gn_edge_bwd_dw_kernel, dim3(tq.grid), dim3(RT_THREADS), 0, st, g, tq.rb, stats, ab, dOut, argk, dw);
    hipLaunchKernelGGL(gn_edge_bwd_du_kernel, dim3(tk.grid), dim3(RT_THREADS), 0, st, g, tk.rb, stats, ab, dOut, argk, rev_off, rev_ent, du);
    return mlsp_launch_status();
}
