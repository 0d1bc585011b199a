// Segmentation supervision on the device (PointSegDA/trainer.py:221-233, 253-258, 309-319): nn.CrossEntropyLoss on the head's [B][N][C]
// logits, their arg-max, and per cloud the macro-averaged IoU (sklearn's jaccard_score) and the accuracy -- the bodies are the phase
// functions of segsup_body.h (tools/segsup_host_check runs them on the host), the arithmetic and its order are stated there.
//   forward   seg_ce_fwd_kernel: workgroup = (cloud, chunk of 256 ppt points), one read of the logits (16-byte quads where C % 4 == 0 and the
//             rows are aligned), lse / loss / pred per point, the chunk's loss sum and integer counters -> workspace
//             seg_finalise_kernel: B + 1 small workgroups: cloud b's sums over its chunks, ascending -> stats[b]; the last one the batch mean
//   metrics   seg_count_kernel (labels and given preds -> the same counters) + the same finaliser
//   backward  seg_ce_bwd_kernel: dlogits = (exp(x - lse) - [c == label]) g, recomputed from the logits and lse; nothing of size C is saved
// Traffic per point: forward 4 C + 8 (label) B read, 8 (lse) + 8 (pred) [+ 4 (loss)] B written; backward 4 C + 16 [+ 4] B read, 4 C written.
// Integer counters use LDS atomics (adds commute); every floating-point sum is taken in double in a fixed order; no float atomics: results
// are bit-identical run to run.  The work is launch-bound at the trainer's shapes (32768 points): two launches forward, one backward.
#include "common.h"
#include "segsup_body.h"

struct SsFwdArgs {
    const float* logits; const long long* labels; double* lse; float* loss_pt; long long* pred; double* csum; int* ccnt;
};

// what both chunk kernels do after their points: the counters (and the loss sum) of chunk `ck` -> workspace
__device__ __forceinline__ void ss_store_counters(const SsGeo& g, int ck, const int* cnt, int* ccnt) {
    const int nc = ss_ncnt(g.C);
    if ((int)threadIdx.x < nc) ccnt[(size_t)ck * nc + threadIdx.x] = cnt[threadIdx.x];
}

template <int NQ, bool VEC>
__global__ __launch_bounds__(SS_THREADS) void seg_ce_fwd_kernel(SsGeo g, SsFwdArgs a) {
    __shared__ int cnt[2 + 3 * SS_MAXC];
    __shared__ double part[SS_THREADS], lead[SS_LEADERS];
    const int tid = threadIdx.x, b = blockIdx.x / g.nch, k = blockIdx.x - b * g.nch;
    if (tid < ss_ncnt(g.C)) ss_zero(tid, cnt);
    __syncthreads();
    part[tid] = ss_thread_points(g, b, k, tid, [&](size_t row) {
        return ss_fwd_point<NQ, VEC>(g, row, a.logits, a.labels, a.lse, a.loss_pt, a.pred, cnt);
    });
    __syncthreads();
    if (tid < SS_LEADERS) ss_sum_leader(part, tid, lead);
    __syncthreads();
    if (tid == 0) a.csum[blockIdx.x] = ss_sum_chunk(lead);
    ss_store_counters(g, blockIdx.x, cnt, a.ccnt);
}

__global__ __launch_bounds__(SS_THREADS) void seg_count_kernel(SsGeo g, const long long* __restrict__ labels, const long long* __restrict__ preds,
                                                               int* __restrict__ ccnt) {
    __shared__ int cnt[2 + 3 * SS_MAXC];
    const int tid = threadIdx.x, b = blockIdx.x / g.nch, k = blockIdx.x - b * g.nch;
    if (tid < ss_ncnt(g.C)) ss_zero(tid, cnt);
    __syncthreads();
    ss_thread_points(g, b, k, tid, [&](size_t row) { ss_count_point(g, row, labels, preds, cnt); return 0.0; });
    __syncthreads();
    ss_store_counters(g, blockIdx.x, cnt, ccnt);
}

// workgroup b < B: cloud b;  workgroup B: the batch row
__global__ __launch_bounds__(SS_THREADS) void seg_finalise_kernel(SsGeo g, const double* __restrict__ csum, const int* __restrict__ ccnt,
                                                                  double* __restrict__ stats, float* __restrict__ mean) {
    __shared__ int cnt[2 + 3 * SS_MAXC];
    __shared__ double slot_loss[SS_THREADS], slot_valid[SS_THREADS], iou_buf[SS_MAXC];
    const int tid = threadIdx.x, b = blockIdx.x;
    if (b < g.B) {
        if (tid < ss_ncnt(g.C)) cnt[tid] = ss_fin_counter(g, b, tid, ccnt);
        __syncthreads();
        if (tid == 0) ss_fin_cloud(g, b, cnt, ss_fin_loss(g, b, csum), iou_buf, stats);
        return;
    }
    double loss = 0.0, valid = 0.0;
    for (int b0 = 0; b0 < g.B; b0 += SS_THREADS) {             // (uniform trip count)
        const int nb = g.B - b0 < SS_THREADS ? g.B - b0 : SS_THREADS;
        if (tid < nb) { slot_loss[tid] = ss_fin_loss(g, b0 + tid, csum); slot_valid[tid] = (double)ss_fin_counter(g, b0 + tid, 0, ccnt); }
        __syncthreads();
        if (tid == 0) ss_fin_batch_add(slot_loss, slot_valid, nb, loss, valid);
        __syncthreads();
    }
    if (tid == 0) ss_fin_batch(g, loss, valid, stats, mean);
}

template <bool VEC>
__global__ __launch_bounds__(RT_THREADS) void seg_ce_bwd_kernel(SsGeo g, int rb, int c4, const float* __restrict__ logits,
                                                                const long long* __restrict__ labels, const double* __restrict__ lse,
                                                                const float* __restrict__ g_pt, const float* __restrict__ g_mean,
                                                                const double* __restrict__ stats, float* __restrict__ dlogits) {
    const long long rows = (long long)g.B * g.N;
    const float gm = g_pt ? 0.f : ss_mean_scale(g, g_mean, stats);
    RT_FOR_ITEMS(rows, rb, c4, RT_THREADS) {
        const int lr = it_ / c4;
        if (VEC) ss_bwd_quad(g, (size_t)(r0_ + lr), it_ - lr * c4, logits, labels, lse, g_pt, gm, dlogits);
        else ss_bwd_scalar(g, (size_t)(r0_ + lr), it_ - lr * c4, logits, labels, lse, g_pt, gm, dlogits);
    }
}

static int launch_seg_finalise(hipStream_t st, const SsGeo& g, const double* csum, const int* ccnt, double* stats, float* mean) {
    hipLaunchKernelGGL(seg_finalise_kernel, dim3(g.B + 1), dim3(SS_THREADS), 0, st, g, csum, ccnt, stats, mean);
    return mlsp_launch_status();
}
template <int NQ>
static int launch_seg_fwd_nq(hipStream_t st, const SsGeo& g, const SsFwdArgs& a) {
    const dim3 grid((unsigned)(g.B * g.nch));
    if (g.vec) hipLaunchKernelGGL((seg_ce_fwd_kernel<NQ, true>), grid, dim3(SS_THREADS), 0, st, g, a);
    else hipLaunchKernelGGL((seg_ce_fwd_kernel<NQ, false>), grid, dim3(SS_THREADS), 0, st, g, a);
    return mlsp_launch_status();
}

size_t seg_ws_bytes(int B, int N, int C) {
    SsGeo g;
    return ss_geo(B, N, C, C, nullptr, g) ? align_up(ss_ws_bytes(g), 256) + MLSP_AMAX_TAIL_BYTES : 0;
}

int launch_seg_ce_fwd(hipStream_t st, const float* logits, int ld, const long long* labels, int B, int N, int C, double* lse, float* loss_pt,
                      long long* pred, double* stats, float* mean, Workspace& ws) {
    SsGeo g;
    if (!ss_geo(B, N, C, ld, logits, g) || (long long)B * g.nch >= (1ll << 31)) return MLSP_ERR_UNSUPPORTED;
    if (!logits || !labels || !lse || !pred || !stats) return MLSP_ERR_ARG;
    char* base = ws.take<char>(ss_ws_bytes(g));
    if (!base) return MLSP_ERR_WORKSPACE;
    SsFwdArgs a;
    a.logits = logits; a.labels = labels; a.lse = lse; a.loss_pt = loss_pt; a.pred = pred;
    a.csum = (double*)base; a.ccnt = (int*)(base + ss_ws_cnt_offset(g));
    const int rc = C <= 4 * SS_REGQ ? launch_seg_fwd_nq<SS_REGQ>(st, g, a) : launch_seg_fwd_nq<0>(st, g, a);
    if (rc != MLSP_OK) return rc;
    return launch_seg_finalise(st, g, a.csum, a.ccnt, stats, mean);
}

int launch_seg_metrics(hipStream_t st, const long long* labels, const long long* preds, int B, int N, int C, double* stats, Workspace& ws) {
    SsGeo g;
    if (!ss_geo(B, N, C, C, nullptr, g) || (long long)B * g.nch >= (1ll << 31)) return MLSP_ERR_UNSUPPORTED;
    if (!labels || !preds || !stats) return MLSP_ERR_ARG;
    char* base = ws.take<char>(ss_ws_bytes(g));
    if (!base) return MLSP_ERR_WORKSPACE;
    int* ccnt = (int*)(base + ss_ws_cnt_offset(g));
    hipLaunchKernelGGL(seg_count_kernel, dim3((unsigned)(g.B * g.nch)), dim3(SS_THREADS), 0, st, g, labels, preds, ccnt);
    const int rc = mlsp_launch_status();
    if (rc != MLSP_OK) return rc;
    return launch_seg_finalise(st, g, nullptr, ccnt, stats, nullptr);
}

// g_pt [B N] (reduction 'none') or g_mean [1] with the forward's stats (reduction 'mean'): exactly one of the two
int launch_seg_ce_bwd(hipStream_t st, const float* logits, int ld, const long long* labels, const double* lse, int B, int N, int C,
                      const float* g_pt, const float* g_mean, const double* stats, float* dlogits) {
    SsGeo g;
    if (!ss_geo(B, N, C, ld, logits, g)) return MLSP_ERR_UNSUPPORTED;
    if (!logits || !labels || !lse || !dlogits || (g_pt != nullptr) == (g_mean != nullptr) || (g_mean && !stats)) return MLSP_ERR_ARG;
    const bool vec = g.vec && al16(dlogits);
    const int c4 = vec ? C / 4 : C;
    const RowTiles t = row_tiles((long long)B * N, c4);
    if (vec) hipLaunchKernelGGL(seg_ce_bwd_kernel<true>, dim3(t.grid), dim3(RT_THREADS), 0, st, g, t.rb, c4, logits, labels, lse, g_pt, g_mean, stats, dlogits);
    else hipLaunchKernelGGL(seg_ce_bwd_kernel<false>, dim3(t.grid), dim3(RT_THREADS), 0, st, g, t.rb, c4, logits, labels, lse, g_pt, g_mean, stats, dlogits);
    return mlsp_launch_status();
}
