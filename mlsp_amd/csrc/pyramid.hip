// The two stages of the Point Transformer models (PointDA/hengshuang_transformer/hengshuang_model.py) that no other op covers.  The bodies
// are the phase functions of pyramid_body.h (tools/pyramid_host_check runs them on the host).
//
// Upsample-and-add: TransitionUp's feats2 + three-nearest-neighbour interpolation of feats1 in one pass -- the interpolated [B][N][C]
// tensor and the addition that followed it do not exist.  Weights and summation order are interp3_fwd_kernel's (sa.hip).  The backward
// gathers dfeat over the reverse index (one writer per element); with one source row per cloud both directions are a broadcast / a sum.
// Cloud mean: points.mean(1), [B N][C] -> [B][C], rows added in double in a fixed order; its backward writes dX completely.
// fp32, channels contiguous, a thread owns 4 channels, wave64, 64-bit element offsets, no atomics: bit-identical run to run.
// Traffic per output element: forward 4 B read (add) + 4 B written, the three source rows from cache (S <= N / 4 in these models).
// Bounds: C % 4 == 0, 16-byte-aligned pointers; idx entries in [0, S) and reverse lists as mlsp_group_reverse leaves them (the caller's
// contract, as for mlsp_interp3_*_f32).
#include "common.h"
#include "pyramid_body.h"

__global__ __launch_bounds__(RT_THREADS) void interp3_add_fwd_kernel(PyGeo g, int rb, const float* __restrict__ feat, const int* __restrict__ idx,
                                                                     const float* __restrict__ dist, const float* __restrict__ add,
                                                                     float* __restrict__ out) {
    const long long rows = (long long)g.B * g.N;
    RT_FOR_ITEMS(rows, rb, g.c4, RT_THREADS) {
        const int lr = it_ / g.c4;
        py_interp_add_fwd_item(g, r0_ + lr, it_ - lr * g.c4, feat, idx, dist, add, out);
    }
}
__global__ __launch_bounds__(RT_THREADS) void interp3_add_bwd_kernel(PyGeo g, int rb, const float* __restrict__ dout, const float* __restrict__ dist,
                                                                     const int* __restrict__ rev_off, const int* __restrict__ rev_ent,
                                                                     float* __restrict__ dfeat) {
    const long long rows = (long long)g.B * g.S;
    RT_FOR_ITEMS(rows, rb, g.c4, RT_THREADS) {
        const int lr = it_ / g.c4;
        py_interp_add_bwd_item(g, r0_ + lr, it_ - lr * g.c4, dout, dist, rev_off, rev_ent, dfeat);
    }
}
// workgroup (b, quad block) = blockIdx.x / nqb, blockIdx.x % nqb
__global__ __launch_bounds__(RT_THREADS) void cloud_sum_kernel(PyGeo g, double div, const float* __restrict__ X, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double sh[RT_THREADS * 4];
    const int b = blockIdx.x / g.nqb, cq0 = (blockIdx.x - b * g.nqb) * g.ct;
    py_cloud_sum_1(g, b, cq0, threadIdx.x, X, sh);
    __syncthreads();
    py_cloud_sum_2(g, b, cq0, threadIdx.x, sh, div, out);
}
__global__ __launch_bounds__(RT_THREADS) void cloud_mean_bwd_kernel(PyGeo g, int rb, const float* __restrict__ dOut, float* __restrict__ dX) {
    const long long rows = (long long)g.B * g.N;
    RT_FOR_ITEMS(rows, rb, g.c4, RT_THREADS) {
        const int lr = it_ / g.c4;
        py_cloud_mean_bwd_item(g, r0_ + lr, it_ - lr * g.c4, dOut, dX);
    }
}

int launch_interp3_add_fwd(hipStream_t st, const float* feat, const int* idx, const float* dist, const float* add, int B, int N, int S, int C,
                           float* out) {
    PyGeo g;
    if (!py_geo(B, N, S, C, g) || S == 2 || !al16(feat, add, out)) return MLSP_ERR_UNSUPPORTED;
    const RowTiles t = row_tiles((long long)B * N, g.c4);
    hipLaunchKernelGGL(interp3_add_fwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, g, t.rb, feat, idx, dist, add, out);
    return mlsp_launch_status();
}
int launch_interp3_add_bwd(hipStream_t st, const float* dout, const float* dist, const int* rev_off, const int* rev_ent, int B, int N, int S,
                           int C, float* dfeat) {
    PyGeo g;
    if (!py_geo(B, N, S, C, g) || S == 2 || !al16(dout, dfeat)) return MLSP_ERR_UNSUPPORTED;
    if (S == 1) {                                           // dfeat[b] = the sum of the cloud's rows of dout
        hipLaunchKernelGGL(cloud_sum_kernel, dim3(B * g.nqb), dim3(RT_THREADS), 0, st, g, 1.0, dout, dfeat);
        return mlsp_launch_status();
    }
    const RowTiles t = row_tiles((long long)B * S, g.c4);
    hipLaunchKernelGGL(interp3_add_bwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, g, t.rb, dout, dist, rev_off, rev_ent, dfeat);
    return mlsp_launch_status();
}
int launch_cloud_mean_fwd(hipStream_t st, const float* X, int B, int N, int C, float* out) {
    PyGeo g;
    if (!py_geo(B, N, 1, C, g) || !al16(X, out)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cloud_sum_kernel, dim3(B * g.nqb), dim3(RT_THREADS), 0, st, g, (double)N, X, out);
    return mlsp_launch_status();
}
int launch_cloud_mean_bwd(hipStream_t st, const float* dOut, int B, int N, int C, float* dX) {
    PyGeo g;
    if (!py_geo(B, N, 1, C, g) || !al16(dOut, dX)) return MLSP_ERR_UNSUPPORTED;
    const RowTiles t = row_tiles((long long)B * N, g.c4);
    hipLaunchKernelGGL(cloud_mean_bwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, g, t.rb, dOut, dX);
    return mlsp_launch_status();
}
