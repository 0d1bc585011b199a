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

// rows x c4 work items in tiles of `rb` rows: a workgroup strides the tiles, its threads the items of a tile
#define PY_ITEM_LOOP(rows_, call_)                                                                                       \
    for (long long r0 = (long long)blockIdx.x * rb; r0 < (rows_); r0 += (long long)gridDim.x * rb) {                     \
        const int n_ = (int)(((rows_) - r0 < rb ? (rows_) - r0 : (long long)rb) * g.c4);                                 \
        for (int it = threadIdx.x; it < n_; it += PY_THREADS) {                                                          \
            const int lr = it / g.c4;                                                                                    \
            const long long r = r0 + lr;                                                                                 \
            const int cq = it - lr * g.c4;                                                                               \
            call_;                                                                                                       \
        }                                                                                                                \
    }

__global__ __launch_bounds__(PY_THREADS) void interp3_add_fwd_kernel(PyGeo g, int rb, const float* __restrict__ feat, const int* __restrict__ idx,
                                                                     const float* __restrict__ dist, const float* __restrict__ add,
                                                                     float* __restrict__ out) {
    const long long rows = (long long)g.B * g.N;
    PY_ITEM_LOOP(rows, py_interp_add_fwd_item(g, r, cq, feat, idx, dist, add, out))
}
__global__ __launch_bounds__(PY_THREADS) void interp3_add_bwd_kernel(PyGeo g, int rb, const float* __restrict__ dout, const float* __restrict__ dist,
                                                                     const int* __restrict__ rev_off, const int* __restrict__ rev_ent,
                                                                     float* __restrict__ dfeat) {
    const long long rows = (long long)g.B * g.S;
    PY_ITEM_LOOP(rows, py_interp_add_bwd_item(g, r, cq, dout, dist, rev_off, rev_ent, dfeat))
}
// workgroup (b, quad block) = blockIdx.x / nqb, blockIdx.x % nqb
__global__ __launch_bounds__(PY_THREADS) void cloud_sum_kernel(PyGeo g, double div, const float* __restrict__ X, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) double sh[PY_THREADS * 4];
    const int b = blockIdx.x / g.nqb, cq0 = (blockIdx.x - b * g.nqb) * g.ct;
    py_cloud_sum_1(g, b, cq0, threadIdx.x, X, sh);
    __syncthreads();
    py_cloud_sum_2(g, b, cq0, threadIdx.x, sh, div, out);
}
__global__ __launch_bounds__(PY_THREADS) void cloud_mean_bwd_kernel(PyGeo g, int rb, const float* __restrict__ dOut, float* __restrict__ dX) {
    const long long rows = (long long)g.B * g.N;
    PY_ITEM_LOOP(rows, py_cloud_mean_bwd_item(g, r, cq, dOut, dX))
}

#define PY_GRID_MAX (1 << 20)
static inline bool py_al(const void* p) { return ((uintptr_t)p & 15) == 0; }
// tiles of about 1024 items
static inline int py_rb(const PyGeo& g) { return g.c4 >= 1024 ? 1 : 1024 / g.c4; }
static inline dim3 py_grid(long long rows, int rb) {
    const long long ntiles = (rows + rb - 1) / rb;
    return dim3((unsigned)(ntiles < PY_GRID_MAX ? ntiles : PY_GRID_MAX));
}

int launch_interp3_add_fwd(hipStream_t st, const float* feat, const int* idx, const float* dist, const float* add, int B, int N, int S, int C,
                           float* out) {
    PyGeo g;
    if (!py_geo(B, N, S, C, g) || S == 2 || !py_al(feat) || !py_al(add) || !py_al(out)) return MLSP_ERR_UNSUPPORTED;
    const int rb = py_rb(g);
    hipLaunchKernelGGL(interp3_add_fwd_kernel, py_grid((long long)B * N, rb), dim3(PY_THREADS), 0, st, g, rb, feat, idx, dist, add, out);
    return mlsp_launch_status();
}
int launch_interp3_add_bwd(hipStream_t st, const float* dout, const float* dist, const int* rev_off, const int* rev_ent, int B, int N, int S,
                           int C, float* dfeat) {
    PyGeo g;
    if (!py_geo(B, N, S, C, g) || S == 2 || !py_al(dout) || !py_al(dfeat)) return MLSP_ERR_UNSUPPORTED;
    if (S == 1) {                                           // dfeat[b] = the sum of the cloud's rows of dout
        hipLaunchKernelGGL(cloud_sum_kernel, dim3(B * g.nqb), dim3(PY_THREADS), 0, st, g, 1.0, dout, dfeat);
        return mlsp_launch_status();
    }
    const int rb = py_rb(g);
    hipLaunchKernelGGL(interp3_add_bwd_kernel, py_grid((long long)B * S, rb), dim3(PY_THREADS), 0, st, g, rb, dout, dist, rev_off, rev_ent, dfeat);
    return mlsp_launch_status();
}
int launch_cloud_mean_fwd(hipStream_t st, const float* X, int B, int N, int C, float* out) {
    PyGeo g;
    if (!py_geo(B, N, 1, C, g) || !py_al(X) || !py_al(out)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cloud_sum_kernel, dim3(B * g.nqb), dim3(PY_THREADS), 0, st, g, (double)N, X, out);
    return mlsp_launch_status();
}
int launch_cloud_mean_bwd(hipStream_t st, const float* dOut, int B, int N, int C, float* dX) {
    PyGeo g;
    if (!py_geo(B, N, 1, C, g) || !py_al(dOut) || !py_al(dX)) return MLSP_ERR_UNSUPPORTED;
    const int rb = py_rb(g);
    hipLaunchKernelGGL(cloud_mean_bwd_kernel, py_grid((long long)B * N, rb), dim3(PY_THREADS), 0, st, g, rb, dOut, dX);
    return mlsp_launch_status();
}
