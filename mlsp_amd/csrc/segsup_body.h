// The bodies of the segmentation-supervision kernels (segsup.hip), one function per phase between two workgroup barriers, each a function
// of (thread) or of one point: segsup.hip calls them with threadIdx and a __syncthreads() between phases, tools/segsup_host_check runs
// them on the host, one call per work-item and phase, against exact-size heap buffers.  No lane talks to another inside a phase except
// through the integer counters in LDS (adds commute; the host walk takes a plain increment).
//
// The supervised half of a PointSegDA step (PointSegDA/trainer.py:221-233, 253-258): cross-entropy of [B][N][C] logits with integer labels,
// the arg-max of the same logits and, per cloud, macro-averaged IoU and accuracy -- from ONE read of the logits:
//   point   m = max x, s = sum_c exp(x_c - m): the exps in fp32, their sum and the logarithm in double; lse = m + log s is KEPT in double
//           (an fp32 lse at |x| ~ 1e4 is off by 5e-4, and the backward's softmax exp(x - lse) would carry that as a relative error);
//           loss = lse - x[label], rounded once where it is stored as fp32; pred = the FIRST maximum (strict comparison from c = 0)
//   chunk   SS_THREADS * ppt consecutive points of one cloud: thread t takes the points t, t + 256, ... and adds their losses in double in
//           that order; 16 leaders add 16 threads each, thread 0 adds the 16 leaders -- always ascending.  Counters: valid, correct, and per
//           class tp | true | pred, 32-bit integers
//   cloud   the finaliser adds the chunks in ascending order; mIoU = mean over the classes with true + pred > 0 of tp / (true + pred - tp)
//           in double, summed in numpy's order (ss_sum_numpy) -- sklearn's jaccard_score(average='macro') bit for bit; acc = correct / valid
// A label outside [0, C) (torch's ignore_index -100 among them) is never an index: the point adds nothing to any sum or counter, its
// gradient row is 0; its lse and pred are still written.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "rowtile.h"

#define SS_THREADS RT_THREADS
#define SS_MAXC 64
#define SS_MAXCHUNKS 64                                    // chunks per cloud at most: the finaliser's serial sums stay short
#define SS_LEADERS 16
#define SS_STATS 5                                         // doubles per row of `stats`: loss sum | mIoU | accuracy | valid points | mean loss

// counters of a chunk: valid | correct | tp[C] | true[C] | pred[C]
RT_HD int ss_ncnt(int C) { return 2 + 3 * C; }

// a cloud of N points is cut into nch chunks of `chunk` = 256 ppt points (the last one partial); vec: rows are read as 16-byte quads
struct SsGeo { int B, N, C, ld, ppt, chunk, nch, vec; };
RT_HD bool ss_geo(int B, int N, int C, int ld, const void* logits, SsGeo& g) {
    if (B < 1 || N < 1 || C < 1 || C > SS_MAXC || ld < C || (long long)B * N >= (1ll << 31)) return false;
    g.B = B; g.N = N; g.C = C; g.ld = ld;
    g.ppt = (int)(((long long)N + (long long)SS_THREADS * SS_MAXCHUNKS - 1) / ((long long)SS_THREADS * SS_MAXCHUNKS));
    g.chunk = SS_THREADS * g.ppt;
    g.nch = (int)(((long long)N + g.chunk - 1) / g.chunk);      // (N + chunk passes 2^31 for one cloud of 2.1e9 points)
    g.vec = (C % 4 == 0 && ld % 4 == 0 && ((uintptr_t)logits & 15) == 0) ? 1 : 0;
    return true;
}
// bytes of the per-chunk partial results: [B nch] doubles (loss sums), then [B nch][ncnt] ints
RT_HD size_t ss_ws_cnt_offset(const SsGeo& g) { return (((size_t)g.B * g.nch * 8) + 15) & ~(size_t)15; }
RT_HD size_t ss_ws_bytes(const SsGeo& g) { return ss_ws_cnt_offset(g) + (size_t)g.B * g.nch * ss_ncnt(g.C) * 4; }

RT_HD void ss_inc(int* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, 1);
#else
    ++*p;
#endif
}

// ---- a chunk ---------------------------------------------------------------------------------------------------------------------------
// thread t < ncnt
RT_HD void ss_zero(int t, int* cnt) { cnt[t] = 0; }

// one point's counters: label and pred of a VALID point (label in [0, C)); a pred outside [0, C) (only the metrics entry can bring one)
// counts for the label's class and as a miss, for no predicted class
RT_HD void ss_count(int C, int lab, long long pred, int* cnt) {
    ss_inc(cnt);
    ss_inc(cnt + 2 + C + lab);
    if (pred >= 0 && pred < C) ss_inc(cnt + 2 + 2 * C + (int)pred);
    if (pred == lab) { ss_inc(cnt + 1); ss_inc(cnt + 2 + lab); }
}

// row = b N + n.  NQ > 0: the row's logits live in registers, 4 NQ of them (C <= 4 NQ; every loop is unrolled, so no register is indexed
// by a variable).  The slots past C hold -inf: they never win the maximum and their exp(-inf - m) adds an exact 0 to the sum, so only the
// loads are guarded by C.  NQ == 0 (C > 4 SS_REGQ): too many logits to hold without spilling scalars, so the row is walked twice, maximum
// first; the second walk finds the row's 4 C <= 256 bytes in the cache, the memory behind it is still read once.  Both forms add the exps
// in ascending c.  Returns the point's loss in double (0 for an ignored label).
#define SS_REGQ 2
template <int NQ, bool VEC>
RT_HD double ss_fwd_point(const SsGeo& g, size_t row, const float* logits, const long long* labels, double* lse, float* loss_pt,
                          long long* pred, int* cnt) {
    const float* xr = logits + row * (size_t)g.ld;
    const int C = g.C;
    const long long lab = labels[row];
    const bool valid = lab >= 0 && lab < C;
    const int li = valid ? (int)lab : -1;
    float m, xl = 0.f;
    int arg = 0;
    double s = 0.0;
    // strict comparisons from c = 0: the first maximum stays; a NaN never displaces a number
    if constexpr (NQ == 0) {
        m = xr[0];
        if (VEC) {
#pragma unroll 2
            for (int q = 0; q < C / 4; ++q) {
                const rt_f4 v = rt_ld(xr + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (v[e] > m) { m = v[e]; arg = 4 * q + e; }
            }
#pragma unroll 2
            for (int q = 0; q < C / 4; ++q) {
                const rt_f4 v = rt_ld(xr + 4 * q);
#pragma unroll
                for (int e = 0; e < 4; ++e) s += (double)expf(v[e] - m);
            }
        } else {
#pragma unroll 4
            for (int c = 1; c < C; ++c)
                if (xr[c] > m) { m = xr[c]; arg = c; }
#pragma unroll 4
            for (int c = 0; c < C; ++c) s += (double)expf(xr[c] - m);
        }
        if (valid) xl = xr[li];
    } else {
        float x[4 * NQ];
        if (VEC) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                rt_f4 v = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                if (4 * q < C) v = rt_ld(xr + 4 * q);
                x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4 * NQ; ++c) x[c] = c < C ? xr[c] : -INFINITY;
        }
        m = x[0];
#pragma unroll
        for (int c = 1; c < 4 * NQ; ++c)
            if (x[c] > m) { m = x[c]; arg = c; }
#pragma unroll
        for (int c = 0; c < 4 * NQ; ++c) { s += (double)expf(x[c] - m); xl = c == li ? x[c] : xl; }
    }
    const double l = (double)m + log(s);
    lse[row] = l;
    pred[row] = arg;
    double loss = 0.0;
    if (valid) { loss = l - (double)xl; ss_count(C, li, arg, cnt); }
    if (loss_pt) loss_pt[row] = (float)loss;
    return loss;
}

// the metrics entry's point: given label and pred
RT_HD void ss_count_point(const SsGeo& g, size_t row, const long long* labels, const long long* preds, int* cnt) {
    const long long lab = labels[row];
    if (lab >= 0 && lab < g.C) ss_count(g.C, (int)lab, preds[row], cnt);
}

// thread t's points of chunk k of cloud b, ascending; f(row) -> the point's loss
template <class F>
RT_HD double ss_thread_points(const SsGeo& g, int b, int k, int t, F f) {
    double acc = 0.0;
    const long long n0 = (long long)k * g.chunk, n1 = n0 + g.chunk < g.N ? n0 + g.chunk : (long long)g.N;     // (64-bit: N may be 2^31 - 1)
    for (long long n = n0 + t; n < n1; n += SS_THREADS) acc += f((size_t)b * g.N + (size_t)n);
    return acc;
}
// leader t < SS_LEADERS adds the threads 16 t .. 16 t + 15
RT_HD void ss_sum_leader(const double* part, int t, double* lead) {
    double s = part[16 * t];
#pragma unroll
    for (int q = 1; q < 16; ++q) s += part[16 * t + q];
    lead[t] = s;
}
// thread 0
RT_HD double ss_sum_chunk(const double* lead) {
    double s = lead[0];
#pragma unroll
    for (int q = 1; q < SS_LEADERS; ++q) s += lead[q];
    return s;
}

// ---- the finaliser -----------------------------------------------------------------------------------------------------------------------
// counter t < ncnt of cloud b over its chunks
RT_HD int ss_fin_counter(const SsGeo& g, int b, int t, const int* ccnt) {
    const int nc = ss_ncnt(g.C);
    const int* p = ccnt + (size_t)b * g.nch * nc + t;
    int s = 0;
#pragma unroll 4
    for (int k = 0; k < g.nch; ++k) s += p[(size_t)k * nc];
    return s;
}
// the cloud's loss sum, chunks ascending (csum NULL: the metrics entry, 0)
RT_HD double ss_fin_loss(const SsGeo& g, int b, const double* csum) {
    if (!csum) return 0.0;
    double s = csum[(size_t)b * g.nch];
#pragma unroll 4
    for (int k = 1; k < g.nch; ++k) s += csum[(size_t)b * g.nch + k];
    return s;
}
// the sum of a[0 .. n-1], n <= 64, in the order numpy's add.reduce takes (what np.average does inside jaccard_score): below 8 values
// left to right; from 8 on eight running sums r[j] += a[8 i + j], combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the
// n % 8 last values left to right.  A plain ascending sum differs from sklearn in the last bit once 8 classes are present.
RT_HD double ss_sum_numpy(const double* a, int n) {
    if (n < 8) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += a[i];
        return s;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    int i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    }
    double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) s += a[i];
    return s;
}
// thread 0 of cloud b's workgroup: cnt = the cloud's counters -> stats[b]; iou_buf: SS_MAXC doubles of scratch (LDS)
RT_HD void ss_fin_cloud(const SsGeo& g, int b, const int* cnt, double loss_sum, double* iou_buf, double* stats) {
    const int C = g.C;
    int present = 0;
    for (int c = 0; c < C; ++c) {
        const int tp = cnt[2 + c], tr = cnt[2 + C + c], pr = cnt[2 + 2 * C + c];
        if (tr + pr > 0) iou_buf[present++] = (double)tp / (double)((long long)tr + pr - tp);
    }
    const double iou = ss_sum_numpy(iou_buf, present);
    double* o = stats + (size_t)b * SS_STATS;
    o[0] = loss_sum;
    o[1] = iou / (double)present;                            // no valid point: 0 / 0 = NaN
    o[2] = (double)cnt[1] / (double)cnt[0];
    o[3] = (double)cnt[0];
    o[4] = loss_sum / (double)cnt[0];
}
// the batch row stats[B] = mean loss | valid points | 0 | 0 | 0 from the per-cloud sums, clouds ascending (thread 0 of the last workgroup;
// slot_* hold the sums of the clouds b0 .. b0 + nb - 1)
RT_HD void ss_fin_batch_add(const double* slot_loss, const double* slot_valid, int nb, double& loss, double& valid) {
    for (int q = 0; q < nb; ++q) { loss += slot_loss[q]; valid += slot_valid[q]; }
}
RT_HD void ss_fin_batch(const SsGeo& g, double loss, double valid, double* stats, float* mean) {
    double* o = stats + (size_t)g.B * SS_STATS;
    o[0] = loss / valid;                                     // every label ignored: 0 / 0 = NaN, as torch
    o[1] = valid; o[2] = 0.0; o[3] = 0.0; o[4] = 0.0;
    if (mean) *mean = (float)o[0];
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------
// the gradient that multiplies every row under the mean reduction: grad / valid points (in double, rounded once)
RT_HD float ss_mean_scale(const SsGeo& g, const float* g_mean, const double* stats) {
    return (float)((double)*g_mean / stats[(size_t)g.B * SS_STATS + 1]);
}
RT_HD float ss_bwd_value(float x, double l, int c, long long lab, float gr) {
    const float p = expf((float)((double)x - l));
    return (p - (c == lab ? 1.f : 0.f)) * gr;
}
// item (row, quad q) of the vector path / (row, class c) of the scalar path.  dlogits is [B N][C], contiguous
RT_HD void ss_bwd_quad(const SsGeo& g, size_t row, int q, const float* logits, const long long* labels, const double* lse, const float* g_pt,
                       float gm, float* dlogits) {
    const long long lab = labels[row];
    rt_f4 d = {0.f, 0.f, 0.f, 0.f};
    if (lab >= 0 && lab < g.C) {
        const rt_f4 v = rt_ld(logits + row * (size_t)g.ld + 4 * q);
        const double l = lse[row];
        const float gr = g_pt ? g_pt[row] : gm;
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = ss_bwd_value(v[e], l, 4 * q + e, lab, gr);
    }
    rt_st(dlogits + row * (size_t)g.C + 4 * q, d);
}
RT_HD void ss_bwd_scalar(const SsGeo& g, size_t row, int c, const float* logits, const long long* labels, const double* lse, const float* g_pt,
                         float gm, float* dlogits) {
    const long long lab = labels[row];
    float d = 0.f;
    if (lab >= 0 && lab < g.C) d = ss_bwd_value(logits[row * (size_t)g.ld + c], lse[row], c, lab, g_pt ? g_pt[row] : gm);
    dlogits[row * (size_t)g.C + c] = d;
}
