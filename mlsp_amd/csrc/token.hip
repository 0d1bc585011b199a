// The two stages of the Point-BERT PointTransformer (PointDA/Models.py:365-531) that had no kernel.  The bodies are the phase functions of
// token_body.h (tools/token_host_check runs them on the host).
//
// Thin-input layer, H = act(BN?(X W^T + b)) with X [M][Cin], Cin <= 8 (the tokeniser's Conv1d(3,128)+BN+ReLU over every grouped point,
// pos_embed's Linear(3,128)+GELU).  BatchNorm of a linear map of so narrow an input needs no pre-BN tensor: with mu = mean(x) and
// Sigma = cov(x), mean_c = w_c mu + b_c and var_c = w_c^T Sigma w_c.
//   moments    sums of d and d d^T (d = x - row 0) per row chunk, fp64 from the first addition; one finaliser workgroup combines the
//              chunks in ascending order -> xmom = mu | Sigma, bn_save = scale | shift | mean | invstd, the running buffers
//   apply      H = act(gamma invstd_c w_c (x - mu) + beta): the centred form, the bias cancels; a streaming write, nothing else of
//              size M C exists
//   bwd sums   one pass over dH recomputes y from X and sums dz, dz yhat, dz (x - mu) per channel: fp32 partials per workgroup, a
//              finaliser adds them in ascending order in double and forms dgamma, dbeta, dW, db (sum yhat (x - mu) comes from Sigma)
// Token pooling, out[b] = y[b L] | max over rows 1 .. L-1, and its backward, which writes dy completely (one writer per element).
// fp32, channels contiguous, a thread owns 4 channels, wave64, 64-bit element offsets, no atomics, every sum in a fixed order.
// Traffic per output element: apply 4 B written (X and W come from cache); bwd sums 4 B read; pool 4 B read per y element.
// Bounds: Cin <= 8, C % 4 == 0, C <= 4096, d % 4 == 0, L >= 2, 16-byte-aligned H / dH / per-channel vectors / y / out / arg.
#include "common.h"
#include "token_body.h"

template <int KC>
__global__ __launch_bounds__(TK_MOM_THREADS) void thin_in_moments_kernel(TkGeo g, double* __restrict__ part) {
    __shared__ double sh[TK_NMOM * TK_MOM_THREADS];
    tk_mom_1<KC>(g, blockIdx.x, threadIdx.x, sh);
    __syncthreads();
    tk_mom_2(g, blockIdx.x, threadIdx.x, sh, part);
}
// one workgroup; xmom / bn_save are written in one phase and read in the next by other threads of the same workgroup
__global__ __launch_bounds__(RT_THREADS) void thin_in_finalize_kernel(TkGeo g, const double* __restrict__ part, double* xmom, float* bn_save,
                                                                      float* run_mean, float* run_var) {
    __shared__ double sh[TK_NMOM];
    tk_fin_1(g, threadIdx.x, part, sh);
    __syncthreads();
    tk_fin_2(g, threadIdx.x, sh, xmom);
    __threadfence_block();
    __syncthreads();
    tk_fin_3(g, threadIdx.x, xmom, bn_save, run_mean, run_var);
}
__global__ __launch_bounds__(RT_THREADS) void thin_in_running_kernel(TkGeo g, const float* __restrict__ run_mean, const float* __restrict__ run_var,
                                                                     float* __restrict__ bn_save) {
    tk_running_item(g, blockIdx.x * RT_THREADS + threadIdx.x, run_mean, run_var, bn_save);
}
template <int KC, int MODE>
__global__ __launch_bounds__(RT_THREADS) void thin_in_apply_kernel(TkGeo g, const float* __restrict__ bn_save, const double* __restrict__ xmom,
                                                                   float* __restrict__ H) {
    tk_apply<KC, MODE>(g, blockIdx.x, blockIdx.y * g.ct, threadIdx.x, bn_save, xmom, H);
}
template <int KC, int MODE>
__global__ __launch_bounds__(RT_THREADS) void thin_in_bwd_sums_kernel(TkGeo g, const float* __restrict__ bn_save, const double* __restrict__ xmom,
                                                                      const float* __restrict__ dH, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sh[RT_THREADS * (2 + KC) * 4];
    tk_bwd_1<KC, MODE>(g, blockIdx.x, blockIdx.y * g.ct, threadIdx.x, bn_save, xmom, dH, sh);
    __syncthreads();
    tk_bwd_2(g, blockIdx.x, blockIdx.y * g.ct, threadIdx.x, sh, part);
}
__global__ __launch_bounds__(RT_THREADS) void thin_in_bwd_finalize_kernel(TkGeo g, const float* __restrict__ part, const float* __restrict__ bn_save,
                                                                          const double* __restrict__ xmom, float* __restrict__ dW,
                                                                          float* __restrict__ db, float* __restrict__ dgamma,
                                                                          float* __restrict__ dbeta) {
    tk_bwd_fin(g, blockIdx.x * RT_THREADS + threadIdx.x, part, bn_save, xmom, dW, db, dgamma, dbeta);
}

// workgroup (b, quad block) = blockIdx.x / nqb, blockIdx.x % nqb
__global__ __launch_bounds__(RT_THREADS) void token_pool_fwd_kernel(TpGeo g, const float* __restrict__ y, float* __restrict__ out,
                                                                    int* __restrict__ arg) {
    __shared__ __attribute__((aligned(16))) float sh_v[RT_THREADS * 4];
    __shared__ __attribute__((aligned(16))) int sh_a[RT_THREADS * 4];
    const int b = blockIdx.x / g.nqb, cq0 = (blockIdx.x - b * g.nqb) * g.ct;
    tp_fwd_1(g, b, cq0, threadIdx.x, y, sh_v, sh_a);
    __syncthreads();
    tp_fwd_2(g, b, cq0, threadIdx.x, y, sh_v, sh_a, out, arg);
}
__global__ __launch_bounds__(RT_THREADS) void token_pool_bwd_kernel(TpGeo g, int rb, const float* __restrict__ dOut, const int* __restrict__ arg,
                                                                    float* __restrict__ dy) {
    const long long rows = (long long)g.B * g.L;
    RT_FOR_ITEMS(rows, rb, g.c4, RT_THREADS) {
        const int lr = it_ / g.c4;
        tp_bwd_item(g, r0_ + lr, it_ - lr * g.c4, dOut, arg, dy);
    }
}

// ---------------------------------------------------------------------------------------------
// Grids of the apply and backward-sum kernels: x = row chunk, y = block of ct channel quads.  TK_PICK: the (input width, mode) variant.
#define TK_PICK(kern_, g_, np_, ...)                                                                                                         \
    do {                                                                                                                                  \
        const dim3 grid_((np_), ((g_).c4 + (g_).ct - 1) / (g_).ct);                                                                     \
        if ((g_).kc == 4) {                                                                                                               \
            if ((g_).mode == TK_MODE_BATCH) hipLaunchKernelGGL((kern_<4, TK_MODE_BATCH>), grid_, dim3(RT_THREADS), 0, st, __VA_ARGS__);   \
            else if ((g_).mode == TK_MODE_RUNNING) hipLaunchKernelGGL((kern_<4, TK_MODE_RUNNING>), grid_, dim3(RT_THREADS), 0, st, __VA_ARGS__); \
            else hipLaunchKernelGGL((kern_<4, TK_MODE_PLAIN>), grid_, dim3(RT_THREADS), 0, st, __VA_ARGS__);                              \
        } else {                                                                                                                          \
            if ((g_).mode == TK_MODE_BATCH) hipLaunchKernelGGL((kern_<8, TK_MODE_BATCH>), grid_, dim3(RT_THREADS), 0, st, __VA_ARGS__);   \
            else if ((g_).mode == TK_MODE_RUNNING) hipLaunchKernelGGL((kern_<8, TK_MODE_RUNNING>), grid_, dim3(RT_THREADS), 0, st, __VA_ARGS__); \
            else hipLaunchKernelGGL((kern_<8, TK_MODE_PLAIN>), grid_, dim3(RT_THREADS), 0, st, __VA_ARGS__);                              \
        }                                                                                                                                 \
    } while (0)
static inline bool tk_setup(const float* X, int ldx, int M, int Cin, const float* W, const float* bias, int C, const float* gamma, const float* beta,
                            int training, int act, float eps, float momentum, TkGeo& g) {
    const int mode = !gamma ? TK_MODE_PLAIN : training ? TK_MODE_BATCH : TK_MODE_RUNNING;
    if (!tk_geo(M, Cin, C, ldx, act, mode, eps, momentum, g) || !al16(bias, gamma, beta)) return false;
    g.X = X; g.W = W; g.bias = bias; g.gamma = gamma; g.beta = beta;
    return true;
}
size_t thin_in_ws_bytes(int M, int Cin, int C) {
    TkGeo g;
    if (!tk_geo(M, Cin, C, Cin, TK_ACT_NONE, TK_MODE_BATCH, 0.f, 0.f, g)) return 0;
    const size_t fwd = align_up(tk_fwd_ws_doubles(g) * sizeof(double), 256), bwd = align_up(tk_bwd_ws_floats(g) * sizeof(float), 256);
    return (fwd > bwd ? fwd : bwd) + MLSP_AMAX_TAIL_BYTES;
}
int launch_thin_in_fwd(hipStream_t st, const float* X, int ldx, int M, int Cin, const float* W, const float* bias, int C, const float* gamma,
                       const float* beta, float* run_mean, float* run_var, float momentum, float eps, int training, int act, float* H,
                       float* bn_save, double* xmom, Workspace& ws) {
    TkGeo g;
    if (!tk_setup(X, ldx, M, Cin, W, bias, C, gamma, beta, training, act, eps, momentum, g) || !al16(H, bn_save)) return MLSP_ERR_UNSUPPORTED;
    if (g.mode == TK_MODE_BATCH) {
        double* part = ws.take<double>(tk_fwd_ws_doubles(g));
        if (!ws.ok()) return MLSP_ERR_WORKSPACE;
        if (g.kc == 4) hipLaunchKernelGGL(thin_in_moments_kernel<4>, dim3(g.m_np), dim3(TK_MOM_THREADS), 0, st, g, part);
        else hipLaunchKernelGGL(thin_in_moments_kernel<8>, dim3(g.m_np), dim3(TK_MOM_THREADS), 0, st, g, part);
        hipLaunchKernelGGL(thin_in_finalize_kernel, dim3(1), dim3(RT_THREADS), 0, st, g, part, xmom, bn_save, run_mean, run_var);
    } else if (g.mode == TK_MODE_RUNNING) {
        hipLaunchKernelGGL(thin_in_running_kernel, dim3((C + RT_THREADS - 1) / RT_THREADS), dim3(RT_THREADS), 0, st, g, run_mean, run_var, bn_save);
    }
    TK_PICK(thin_in_apply_kernel, g, g.a_np, g, bn_save, xmom, H);
    return mlsp_launch_status();
}
int launch_thin_in_bwd(hipStream_t st, const float* dH, const float* X, int ldx, int M, int Cin, const float* W, const float* bias, int C,
                       const float* gamma, const float* beta, const float* bn_save, const double* xmom, int training, int act, float* dW,
                       float* db, float* dgamma, float* dbeta, Workspace& ws) {
    TkGeo g;
    if (!tk_setup(X, ldx, M, Cin, W, bias, C, gamma, beta, training, act, 0.f, 0.f, g) || !al16(dH, bn_save)) return MLSP_ERR_UNSUPPORTED;
    float* part = ws.take<float>(tk_bwd_ws_floats(g));
    if (!ws.ok()) return MLSP_ERR_WORKSPACE;
    TK_PICK(thin_in_bwd_sums_kernel, g, g.b_np, g, bn_save, xmom, dH, part);
    hipLaunchKernelGGL(thin_in_bwd_finalize_kernel, dim3((C + RT_THREADS - 1) / RT_THREADS), dim3(RT_THREADS), 0, st, g, part, bn_save, xmom, dW, db,
                       dgamma, dbeta);
    return mlsp_launch_status();
}

int launch_token_pool_fwd(hipStream_t st, const float* y, int B, int L, int d, float* out, int* arg) {
    TpGeo g;
    if (!tp_geo(B, L, d, g) || !al16(y, out, arg)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(token_pool_fwd_kernel, dim3(B * g.nqb), dim3(RT_THREADS), 0, st, g, y, out, arg);
    return mlsp_launch_status();
}
int launch_token_pool_bwd(hipStream_t st, const float* dOut, const int* arg, int B, int L, int d, float* dy) {
    TpGeo g;
    if (!tp_geo(B, L, d, g) || !al16(dOut, arg, dy)) return MLSP_ERR_UNSUPPORTED;
    const RowTiles t = row_tiles((long long)B * L, g.c4);
    hipLaunchKernelGGL(token_pool_bwd_kernel, dim3(t.grid), dim3(RT_THREADS), 0, st, g, t.rb, dOut, arg, dy);
    return mlsp_launch_status();
}
