// The bodies of the kernels of gnedge.hip, one function per phase between two workgroup barriers, each a function of (workgroup, thread) or
// of one work item: gnedge.hip calls them with blockIdx / threadIdx and a __syncthreads() between phases, tools/gn_edge_host_check/main.hip
// calls them on the host, one call per work-item and phase, against exact-size heap buffers (no lane talks to another inside a phase: what
// crosses lanes goes through LDS or the workspace and a barrier, so the host walk computes what the GPU computes).  Element offsets into
// global memory are 64-bit.
//
// The edge value is never stored: y(i, s, c) = u[j][c] + w[i][c], j = idx[i][s] local to the cloud of query point i (an index outside
// [0, Nk) is read as 0).  A thread owns 4 channels (one 16-byte access); C % (4 groups) == 0, so its four channels share a GroupNorm group.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "rowtile.h"

#define GE_MAX_K 64
#define GE_MAX_GROUPS 256
#define GE_PARTS_MAX 64                                    // row chunks (workgroups) per cloud of the two summing passes

// u [B Nk][C] (pitch ldu), w [B Nq][C] (pitch ldw), idx [B][Nq][k]; every other [.][C] matrix is contiguous.
// The summing passes: a workgroup is (cloud b, chunk p of `chunk` query rows), its threads (row lane r < rl, channel quad tc < ct).
struct GeGeo {
    int B, Nk, Nq, k, C, c4, groups, gq, ldu, ldw, ct, rl, np, chunk;          // gq: channel quads per group
    float eps, slope;
    double inv_n;                                                               // 1 / (Cg Nq k): the size of a (cloud, group)
    const float *u, *w, *gamma, *beta;
    const int* idx;
};
// the geometry of a shape, or false outside the limits
RT_HD bool ge_geo(int B, int Nk, int Nq, int k, int C, int groups, int ldu, int ldw, float eps, float slope, GeGeo& g) {
    if (B <= 0 || Nk <= 0 || Nq <= 0 || k < 1 || k > GE_MAX_K || C <= 0 || groups < 1 || groups > GE_MAX_GROUPS) return false;
    if (C % (4 * groups) || C > (1 << 20) || ldu < C || ldw < C || ldu % 4 || ldw % 4) return false;
    if (Nk > (1 << 22) || Nq > (1 << 22) || (long long)B * Nk > (1LL << 30) || (long long)B * Nq > (1LL << 30)) return false;
    g.B = B; g.Nk = Nk; g.Nq = Nq; g.k = k; g.C = C; g.c4 = C / 4; g.groups = groups; g.gq = C / 4 / groups; g.ldu = ldu; g.ldw = ldw;
    g.ct = g.c4 < RT_THREADS ? g.c4 : RT_THREADS;
    g.rl = RT_THREADS / g.ct;
    const int want = (Nq + g.rl * 8 - 1) / (g.rl * 8);
    g.np = want < 1 ? 1 : want > GE_PARTS_MAX ? GE_PARTS_MAX : want;
    g.chunk = (Nq + g.np - 1) / g.np;
    g.np = (Nq + g.chunk - 1) / g.chunk;                    // no empty chunk
    g.eps = eps; g.slope = slope;
    g.inv_n = 1.0 / ((double)(C / groups) * Nq * k);
    g.u = g.w = g.gamma = g.beta = nullptr; g.idx = nullptr;
    return (long long)B * g.np < (1LL << 31);
}
// workspace of the forward: part [B][np][groups][2] doubles;  of the backward: chpart [B][np][c4][2] quads | cloud [B][C][2] doubles
RT_HD size_t ge_fwd_ws_doubles(const GeGeo& g) { return (size_t)g.B * g.np * g.groups * 2; }
RT_HD size_t ge_bwd_ws_floats(const GeGeo& g) { return (size_t)g.B * g.np * g.C * 2; }
RT_HD size_t ge_bwd_ws_doubles(const GeGeo& g) { return (size_t)g.B * g.C * 2; }

RT_HD long long ge_src(const GeGeo& g, long long i, int s) {              // the global source row of slot s of query row i
    const int j = g.idx[i * g.k + s];
    return (i / g.Nq) * g.Nk + ((unsigned)j < (unsigned)g.Nk ? j : 0);
}
RT_HD float ge_lrelu(float v, float slope) { return v > 0.f ? v : v * slope; }

// ---------------------------------------------------------------------------------------------
// Statistics of a (cloud, group): sums of y and y^2 in fp64 (a product of two fp32 values is exact in fp64, and the difference
// E[y^2] - E[y]^2 formed there keeps 1e-16 of y^2: nothing an fp32 result sees).
// 1: sh[tid] = {sum y, sum y^2} over the thread's rows, slots and 4 channels;  2: thread g < groups adds the lanes of its group's quads in
// ascending (quad, row lane) to part[b][p][g] (it alone owns that entry over the cq0 steps).  LDS: sh [256][2] doubles.
RT_HD void ge_stats_1(const GeGeo& g, int b, int p, int cq0, int tid, double* sh) {
    const int tc = tid % g.ct, r = tid / g.ct, cq = cq0 + tc;
    double s1 = 0.0, s2 = 0.0;
    if (r < g.rl && cq < g.c4) {
        const int i0 = p * g.chunk, i1 = i0 + g.chunk < g.Nq ? i0 + g.chunk : g.Nq;
        for (int il = i0 + r; il < i1; il += g.rl) {
            const long long i = (long long)b * g.Nq + il;
            const rt_f4 wv = rt_ld(g.w + i * g.ldw + cq * 4);
            for (int s = 0; s < g.k; ++s) {
                const rt_f4 y = rt_ld(g.u + ge_src(g, i, s) * g.ldu + cq * 4) + wv;
                const double a = y.x, c = y.y, d = y.z, e = y.w;
                s1 += (a + c) + (d + e);
                s2 += (a * a + c * c) + (d * d + e * e);
            }
        }
    }
    sh[tid * 2] = s1; sh[tid * 2 + 1] = s2;
}
RT_HD void ge_stats_2(const GeGeo& g, int b, int p, int cq0, int tid, const double* sh, double* part) {
    for (int gr = tid; gr < g.groups; gr += RT_THREADS) {
        double* dst = part + (((size_t)b * g.np + p) * g.groups + gr) * 2;
        double s1 = cq0 ? dst[0] : 0.0, s2 = cq0 ? dst[1] : 0.0;
        const int q0 = gr * g.gq > cq0 ? gr * g.gq : cq0, q1 = (gr + 1) * g.gq < cq0 + g.ct ? (gr + 1) * g.gq : cq0 + g.ct;
        for (int q = q0; q < q1; ++q)
            for (int r = 0; r < g.rl; ++r) {
                s1 += sh[(r * g.ct + q - cq0) * 2]; s2 += sh[(r * g.ct + q - cq0) * 2 + 1];
            }
        dst[0] = s1; dst[1] = s2;
    }
}
// item t = b groups + gr: the chunks in ascending p;  stats[t] = {mean, 1 / sqrt(biased variance + eps)}
RT_HD void ge_stats_fin(const GeGeo& g, long long t, const double* part, float* stats) {
    if (t >= (long long)g.B * g.groups) return;
    const long long b = t / g.groups, gr = t - b * g.groups;
    double s1 = 0.0, s2 = 0.0;
    for (int p = 0; p < g.np; ++p) {
        const double* src = part + ((b * g.np + p) * g.groups + gr) * 2;
        s1 += src[0]; s2 += src[1];
    }
    const double mean = s1 * g.inv_n;
    double var = s2 * g.inv_n - mean * mean;
    if (var < 0.0) var = 0.0;                               // (a NaN stays a NaN)
    stats[t * 2] = (float)mean;
    stats[t * 2 + 1] = (float)(1.0 / sqrt(var + (double)g.eps));
}

// ---------------------------------------------------------------------------------------------
// out[i][c] = max_s lrelu(yhat gamma[c] + beta[c]), yhat = (y - mean) rstd: lrelu o affine is monotone in y, rising for gamma rstd >= 0
// and falling otherwise, so the slot is chosen on y (the maximum or the minimum; a strict comparison, so the first slot wins ties and a
// NaN never moves the choice: argk stays in [0, k)) and the activation runs once.  Item (query row i, quad cq).
RT_HD void ge_apply_item(const GeGeo& g, long long i, int cq, const float* stats, float* out, uint8_t* argk) {
    const float* st = stats + ((i / g.Nq) * g.groups + cq / g.gq) * 2;
    const float mean = st[0], rstd = st[1];
    const rt_f4 wv = rt_ld(g.w + i * g.ldw + cq * 4), ga = rt_ld(g.gamma + cq * 4), be = rt_ld(g.beta + cq * 4);
    rt_f4 best = rt_ld(g.u + ge_src(g, i, 0) * g.ldu + cq * 4) + wv;
    int arg[4] = {0, 0, 0, 0};
    bool up[4];
    for (int e = 0; e < 4; ++e) up[e] = ga[e] * rstd >= 0.f;
    for (int s = 1; s < g.k; ++s) {
        const rt_f4 y = rt_ld(g.u + ge_src(g, i, s) * g.ldu + cq * 4) + wv;
        for (int e = 0; e < 4; ++e)
            if (up[e] ? y[e] > best[e] : y[e] < best[e]) { best[e] = y[e]; arg[e] = s; }
    }
    rt_f4 o;
    for (int e = 0; e < 4; ++e) o[e] = ge_lrelu((best[e] - mean) * rstd * ga[e] + be[e], g.slope);
    rt_st(out + (i * g.c4 + cq) * 4, o);
    uint8_t* a = argk + (i * g.c4 + cq) * 4;
    for (int e = 0; e < 4; ++e) a[e] = (uint8_t)arg[e];
}

// ---------------------------------------------------------------------------------------------
// Backward.  At the selected slot: yhat_sel, dz = dOut lrelu'(yhat_sel gamma + beta) (torch's rule: slope where the argument is <= 0).
struct GeSel { rt_f4 dz, yh; int arg[4]; };
RT_HD GeSel ge_sel(const GeGeo& g, long long i, int cq, float mean, float rstd, const rt_f4& wv, const float* dOut, const uint8_t* argk) {
    GeSel o;
    const rt_f4 ga = rt_ld(g.gamma + cq * 4), be = rt_ld(g.beta + cq * 4), d = rt_ld(dOut + (i * g.c4 + cq) * 4);
    const uint8_t* a = argk + (i * g.c4 + cq) * 4;
    for (int e = 0; e < 4; ++e) {
        o.arg[e] = a[e];
        const int s = a[e] < g.k ? a[e] : 0;                // (a slot a test forced out of range is read as 0, never past the row)
        const float y = g.u[ge_src(g, i, s) * g.ldu + cq * 4 + e] + wv[e];
        o.yh[e] = (y - mean) * rstd;
        o.dz[e] = o.yh[e] * ga[e] + be[e] > 0.f ? d[e] : d[e] * g.slope;
    }
    return o;
}
// Sums over the selected entries per channel: 1: sh[tid] = {sum dz yhat_sel, sum dz} quads over the thread's rows;  2: the row lanes in
// ascending order -> chpart[b][p][cq] = {dgamma quad, dbeta quad}.  LDS: sh [256][2] quads.
RT_HD void ge_bsum_1(const GeGeo& g, int b, int p, int cq0, int tid, const float* stats, const float* dOut, const uint8_t* argk, float* sh) {
    const int tc = tid % g.ct, r = tid / g.ct, cq = cq0 + tc;
    rt_f4 ag = rt_f4{0.f, 0.f, 0.f, 0.f}, ab = rt_f4{0.f, 0.f, 0.f, 0.f};
    if (r < g.rl && cq < g.c4) {
        const float* st = stats + ((size_t)b * g.groups + cq / g.gq) * 2;
        const float mean = st[0], rstd = st[1];
        const int i0 = p * g.chunk, i1 = i0 + g.chunk < g.Nq ? i0 + g.chunk : g.Nq;
        for (int il = i0 + r; il < i1; il += g.rl) {
            const long long i = (long long)b * g.Nq + il;
            const GeSel o = ge_sel(g, i, cq, mean, rstd, rt_ld(g.w + i * g.ldw + cq * 4), dOut, argk);
            ag += o.dz * o.yh;
            ab += o.dz;
        }
    }
    rt_st(sh + (size_t)tid * 8, ag);
    rt_st(sh + (size_t)tid * 8 + 4, ab);
}
RT_HD void ge_bsum_2(const GeGeo& g, int b, int p, int cq0, int tid, const float* sh, float* chpart) {
    const int tc = tid % g.ct, r = tid / g.ct, cq = cq0 + tc;
    if (r != 0 || cq >= g.c4) return;
    rt_f4 ag = rt_ld(sh + (size_t)tid * 8), ab = rt_ld(sh + (size_t)tid * 8 + 4);
    for (int q = 1; q < g.rl; ++q) {
        ag += rt_ld(sh + (size_t)(q * g.ct + tc) * 8);
        ab += rt_ld(sh + (size_t)(q * g.ct + tc) * 8 + 4);
    }
    float* dst = chpart + (((size_t)b * g.np + p) * g.c4 + cq) * 8;
    rt_st(dst, ag);
    rt_st(dst + 4, ab);
}
// A workgroup per cloud.  1: cloud[b][c] = {sum_p dgamma part, sum_p dbeta part} in fp64, ascending p;  2: thread gr < groups:
// ab[b][gr] = {A, Bm} = {mean over the group of gamma dz, of gamma dz yhat}, its channels in ascending order.
RT_HD void ge_bfin_1(const GeGeo& g, int b, int tid, const float* chpart, double* cloud) {
    for (int c = tid; c < g.C; c += RT_THREADS) {
        double sg = 0.0, sb = 0.0;
        for (int p = 0; p < g.np; ++p) {
            const float* q = chpart + (((size_t)b * g.np + p) * g.c4 + c / 4) * 8;
            sg += q[c % 4]; sb += q[4 + c % 4];
        }
        cloud[((size_t)b * g.C + c) * 2] = sg; cloud[((size_t)b * g.C + c) * 2 + 1] = sb;
    }
}
RT_HD void ge_bfin_2(const GeGeo& g, int b, int tid, const double* cloud, float* ab) {
    const int Cg = g.gq * 4;
    for (int gr = tid; gr < g.groups; gr += RT_THREADS) {
        double sa = 0.0, sb = 0.0;
        for (int c = gr * Cg; c < (gr + 1) * Cg; ++c) {
            const double ga = g.gamma[c];
            sa += ga * cloud[((size_t)b * g.C + c) * 2 + 1];
            sb += ga * cloud[((size_t)b * g.C + c) * 2];
        }
        ab[((size_t)b * g.groups + gr) * 2] = (float)(sa * g.inv_n);
        ab[((size_t)b * g.groups + gr) * 2 + 1] = (float)(sb * g.inv_n);
    }
}
// dgamma[c], dbeta[c]: the clouds in ascending order
RT_HD void ge_bfin_param(const GeGeo& g, int c, const double* cloud, float* dgamma, float* dbeta) {
    if (c >= g.C) return;
    double sg = 0.0, sb = 0.0;
    for (int b = 0; b < g.B; ++b) { sg += cloud[((size_t)b * g.C + c) * 2]; sb += cloud[((size_t)b * g.C + c) * 2 + 1]; }
    dgamma[c] = (float)sg; dbeta[c] = (float)sb;
}
// dy(i, s, c) = rstd (gamma dz [s == argk] - A - yhat(i, s, c) Bm), dense over the slots.
// dw[i][c] = sum_s dy in ascending s.  Item (query row i, quad cq).
RT_HD void ge_bwd_dw_item(const GeGeo& g, long long i, int cq, const float* stats, const float* ab, const float* dOut, const uint8_t* argk,
                          float* dw) {
    const size_t bg = (size_t)(i / g.Nq) * g.groups + cq / g.gq;
    const float mean = stats[bg * 2], rstd = stats[bg * 2 + 1], A = ab[bg * 2], Bm = ab[bg * 2 + 1];
    const rt_f4 wv = rt_ld(g.w + i * g.ldw + cq * 4);
    const GeSel o = ge_sel(g, i, cq, mean, rstd, wv, dOut, argk);
    const rt_f4 gd = rt_ld(g.gamma + cq * 4) * o.dz;
    rt_f4 acc = rt_f4{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < g.k; ++s) {
        const rt_f4 yh = (rt_ld(g.u + ge_src(g, i, s) * g.ldu + cq * 4) + wv - mean) * rstd;
        rt_f4 t;
        for (int e = 0; e < 4; ++e) t[e] = ((o.arg[e] == s ? gd[e] : 0.f) - A) - yh[e] * Bm;
        acc += t * rstd;
    }
    rt_st(dw + (i * g.c4 + cq) * 4, acc);
}
// du[j][c] = sum of dy over the edges (i, s) that name source row j, in the order of the reverse index (rev_off [B Nk + 1], rev_ent =
// (i local << 8) | s, ascending: mlsp_group_reverse); a row no edge names gets exactly 0.  Item (source row j, quad cq).
RT_HD void ge_bwd_du_item(const GeGeo& g, long long j, int cq, const float* stats, const float* ab, const float* dOut, const uint8_t* argk,
                          const int* rev_off, const int* rev_ent, float* du) {
    const long long b = j / g.Nk;
    const size_t bg = (size_t)b * g.groups + cq / g.gq;
    const float mean = stats[bg * 2], rstd = stats[bg * 2 + 1], A = ab[bg * 2], Bm = ab[bg * 2 + 1];
    const rt_f4 uv = rt_ld(g.u + j * g.ldu + cq * 4), ga = rt_ld(g.gamma + cq * 4), be = rt_ld(g.beta + cq * 4);
    rt_f4 acc = rt_f4{0.f, 0.f, 0.f, 0.f};
    for (int e = rev_off[j], e1 = rev_off[j + 1]; e < e1; ++e) {
        const int ent = rev_ent[e], s = ent & 255;
        const long long i = b * g.Nq + (ent >> 8);
        const rt_f4 yh = (uv + rt_ld(g.w + i * g.ldw + cq * 4) - mean) * rstd, d = rt_ld(dOut + (i * g.c4 + cq) * 4);
        const uint8_t* a = argk + (i * g.c4 + cq) * 4;
        rt_f4 t;
        for (int q = 0; q < 4; ++q) {
            const float dz = yh[q] * ga[q] + be[q] > 0.f ? d[q] : d[q] * g.slope;
            t[q] = ((a[q] == s ? ga[q] * dz : 0.f) - A) - yh[q] * Bm;
        }
        acc += t * rstd;
    }
    rt_st(du + (j * g.c4 + cq) * 4, acc);
}
