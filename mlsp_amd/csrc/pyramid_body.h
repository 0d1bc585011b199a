// The bodies of the kernels of pyramid.hip, one function per phase between two workgroup barriers, each a function of (workgroup, thread)
// or of one work item: pyramid.hip calls them with blockIdx / threadIdx and a __syncthreads() between phases, tools/pyramid_host_check runs
// them on the host, one call per work-item and phase, against exact-size heap buffers (no lane talks to another inside a phase: what
// crosses lanes goes through LDS and a barrier).  Element offsets are 64-bit.  fp32 rows of C channels, C % 4 == 0; a thread owns one
// channel quad (a 16-byte access).
//
// Upsample-and-add (TransitionUp of hengshuang_model.py): out[b][n] = add[b][n] + sum_{j<3} w_j feat[b][idx[b][n][j]] with the weights of
// interp3_fwd_kernel (sa.hip), w_j = (1 / (d_j + 1e-8)) / sum_j' (1 / (d_j' + 1e-8)), accumulated in the same order; S == 1 broadcasts the
// one source row (idx / dist unread).  Backward: dfeat[b][s] = sum over the reverse list of s (mlsp_group_reverse, entry = n << 8 | j) of
// w_j dout[b][n], in list order; S == 1: the cloud sum of dout.  dadd = dout.
// Cloud mean: out[b] = (1 / N) sum_n X[b N + n], in double from the first addition, rows in a fixed order.  Backward: dX[b N + n] = dOut[b] / N.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "rowtile.h"

#define PY_CT_MAX 16                                       // channel quads per workgroup of the cloud sums (256 bytes of a row)

// B clouds of N rows (and S source rows for the interpolation) of C channels.  ct / nrl / nqb: the cloud sums' workgroup shape -- thread
// (row lane rl < nrl, quad tc < ct), nqb blocks of ct quads per row.
struct PyGeo { int B, N, S, C, c4, ct, nrl, nqb; };
RT_HD bool py_geo(int B, int N, int S, int C, PyGeo& g) {
    if (B < 1 || N < 1 || S < 1 || C < 4 || C % 4 || C > (1 << 20) || N > (1 << 23) || S > (1 << 23)) return false;
    if ((long long)B * N > (1LL << 30) || (long long)B * S > (1LL << 30)) return false;
    g.B = B; g.N = N; g.S = S; g.C = C; g.c4 = C / 4;
    g.ct = g.c4 < PY_CT_MAX ? g.c4 : PY_CT_MAX;
    g.nrl = RT_THREADS / g.ct;
    g.nqb = (g.c4 + g.ct - 1) / g.ct;
    return (long long)B * g.nqb < (1LL << 31);
}

// ---------------------------------------------------------------------------------------------
// Upsample-and-add forward, item (row pn of B N, quad cq): one writer per element.
RT_HD void py_interp_add_fwd_item(const PyGeo& g, long long pn, int cq, const float* feat, const int* idx, const float* dist, const float* add,
                                  float* out) {
    const long long b = pn / g.N;
    rt_f4 acc;
    if (g.S == 1) {
        acc = rt_ld(feat + b * g.C + cq * 4);
    } else {
        float w[3], ws = 0.f;
#pragma unroll
        for (int u = 0; u < 3; ++u) { w[u] = 1.0f / (dist[pn * 3 + u] + 1e-8f); ws += w[u]; }
        acc = rt_f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 3; ++u) {
            const float wu = w[u] / ws;
            acc += rt_ld(feat + (b * g.S + idx[pn * 3 + u]) * g.C + cq * 4) * wu;
        }
    }
    rt_st(out + pn * g.C + cq * 4, rt_ld(add + pn * g.C + cq * 4) + acc);
}
// Backward for S >= 3, item (source row s of B S, quad cq): its reverse list in order, the weight of every entry recomputed from dist.
RT_HD void py_interp_add_bwd_item(const PyGeo& g, long long s, int cq, const float* dout, const float* dist, const int* rev_off, const int* rev_ent,
                                  float* dfeat) {
    const long long b = s / g.S;
    const int e0 = rev_off[s], e1 = rev_off[s + 1];
    rt_f4 acc = rt_f4{0.f, 0.f, 0.f, 0.f};
    for (int e = e0; e < e1; ++e) {
        const int ent = rev_ent[e];
        const long long pn = b * g.N + (ent >> 8);
        const int u = ent & 255;
        float ws = 0.f, wu = 0.f;
#pragma unroll
        for (int v = 0; v < 3; ++v) { const float w = 1.0f / (dist[pn * 3 + v] + 1e-8f); ws += w; wu = v == u ? w : wu; }
        acc += rt_ld(dout + pn * g.C + cq * 4) * (wu / ws);
    }
    rt_st(dfeat + s * g.C + cq * 4, acc);
}

// ---------------------------------------------------------------------------------------------
// Cloud sums.  Workgroup (cloud b, quad block cq0); 1: thread (rl, tc) adds its rows rl, rl + nrl, ... in double -> sh[tid] (a quad of
// doubles);  2: row lane 0 adds the lanes in ascending order and writes out[b] = sum / div (div = N: the mean; div = 1: the sum).
// LDS: sh [256] quads of doubles.
RT_HD void py_cloud_sum_1(const PyGeo& g, int b, int cq0, int tid, const float* X, double* sh) {
    const int tc = tid % g.ct, rl = tid / g.ct, cq = cq0 + tc;
    if (rl >= g.nrl || cq >= g.c4) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int n = rl; n < g.N; n += g.nrl) {
        const rt_f4 v = rt_ld(X + ((long long)b * g.N + n) * g.C + cq * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) sh[(size_t)tid * 4 + e] = s[e];
}
RT_HD void py_cloud_sum_2(const PyGeo& g, int b, int cq0, int tid, const double* sh, double div, float* out) {
    const int tc = tid % g.ct, rl = tid / g.ct, cq = cq0 + tc;
    if (rl != 0 || cq >= g.c4) return;
    double s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = sh[(size_t)tid * 4 + e];
    for (int q = 1; q < g.nrl; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += sh[(size_t)(q * g.ct + tc) * 4 + e];
    rt_f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (float)(s[e] / div);
    rt_st(out + (long long)b * g.C + cq * 4, o);
}
// dX[r] = dOut[r / N] / N, item (row r of B N, quad cq): one writer per element, nothing pre-filled.
RT_HD void py_cloud_mean_bwd_item(const PyGeo& g, long long r, int cq, const float* dOut, float* dX) {
    const rt_f4 d = rt_ld(dOut + (r / g.N) * g.C + cq * 4);
    rt_f4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = d[e] / (float)g.N;
    rt_st(dX + r * g.C + cq * 4, o);
}
