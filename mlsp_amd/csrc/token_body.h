// The bodies of the kernels of token.hip, one function per phase between two workgroup barriers, each a function of (workgroup, thread):
// token.hip calls them with blockIdx / threadIdx and a __syncthreads() between phases, tools/token_host_check/main.hip calls them on the
// host, one call per work-item and phase, against exact-size heap buffers (no lane talks to another inside a phase: what crosses lanes
// goes through LDS or the workspace and a barrier, so the host walk computes what the GPU computes).  Element offsets are 64-bit.
//
// Thin-input layer: H[M][C] = act(BN?(X W^T + b)), X [M][Cin] with Cin <= 8 (pitch ldx), W [C][Cin] contiguous.  A thread owns 4
// channels (one 16-byte access along C) and walks rows; its 4 x Cin weights stay in registers.  Token pooling: out[b] = y[b L] | max over
// the rows 1 .. L-1 of cloud b.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "rowtile.h"

#define TK_MOM_THREADS 64                                  // the moment pass: 44 fp64 accumulators per thread, one wave per workgroup
#define TK_MAX_CIN 8
#define TK_NMOM 44                                         // 8 first + 36 second moments (upper triangle)
#define TK_XMOM 72                                         // xmom: mu[8] | Sigma[8][8] doubles
#define TK_PARTS_MAX 512                                   // row chunks (workgroups) of the two summing passes
#define TK_ACT_NONE 0
#define TK_ACT_RELU 1
#define TK_ACT_GELU 3
#define TK_MODE_PLAIN 0                                    // no BatchNorm
#define TK_MODE_BATCH 1                                    // BatchNorm on batch statistics (training)
#define TK_MODE_RUNNING 2                                  // BatchNorm on the running buffers (eval)

typedef int tk_i4 __attribute__((ext_vector_type(4)));

// Threads of a 256-wide workgroup: (row lane rl < nrl, channel quad tc < ct).  Row chunks: a_* of the apply pass, m_* of the moment
// pass, b_* of the backward sums.  kc: the compile-time input width the kernels run with (4 or 8).
struct TkGeo {
    int M, Cin, C, c4, ldx, kc, ct, nrl, act, mode;
    int a_chunk, a_np, m_chunk, m_np, b_chunk, b_np;
    float eps, momentum;
    const float *X, *W, *bias, *gamma, *beta;              // bias nullable; gamma / beta NULL in TK_MODE_PLAIN
};
RT_HD int tk_ceil_div(long long a, long long b) { return (int)((a + b - 1) / b); }
// the geometry of a shape, or false outside the limits
RT_HD bool tk_geo(int M, int Cin, int C, int ldx, int act, int mode, float eps, float momentum, TkGeo& g) {
    if (M < 1 || M > (1 << 30) || Cin < 1 || Cin > TK_MAX_CIN || ldx < Cin || C < 4 || C % 4 || C > 4096) return false;
    if ((act != TK_ACT_NONE && act != TK_ACT_RELU && act != TK_ACT_GELU) || mode < 0 || mode > 2) return false;
    g.M = M; g.Cin = Cin; g.C = C; g.c4 = C / 4; g.ldx = ldx; g.kc = Cin <= 4 ? 4 : 8; g.act = act; g.mode = mode;
    g.ct = g.c4 < RT_THREADS ? g.c4 : RT_THREADS;
    g.nrl = RT_THREADS / g.ct;
    // apply: about 1024 workgroups at M = 65,536 x C = 128 (8 rows per thread), one row per thread on small M
    long long per = (long long)M / ((long long)g.nrl * 1024);
    per = per < 1 ? 1 : per > 8 ? 8 : per;
    g.a_chunk = (int)(g.nrl * per);
    g.a_np = tk_ceil_div(M, g.a_chunk);
    // moments: 256 rows (4 per thread) per workgroup, at most TK_PARTS_MAX workgroups
    g.m_chunk = tk_ceil_div(M, TK_PARTS_MAX) > 256 ? tk_ceil_div(M, TK_PARTS_MAX) : 256;
    g.m_np = tk_ceil_div(M, g.m_chunk);
    // backward sums: 8 rows per thread, at most TK_PARTS_MAX workgroups; whole row-lane sweeps
    g.b_chunk = tk_ceil_div(M, TK_PARTS_MAX) > g.nrl * 8 ? tk_ceil_div(M, TK_PARTS_MAX) : g.nrl * 8;
    g.b_chunk = tk_ceil_div(g.b_chunk, g.nrl) * g.nrl;
    g.b_np = tk_ceil_div(M, g.b_chunk);
    g.eps = eps; g.momentum = momentum;
    g.X = g.W = g.bias = g.gamma = g.beta = nullptr;
    return true;
}
// workspace: the forward's part [m_np][44] doubles; the backward's part [b_np][c4][2 + kc] quads
RT_HD size_t tk_fwd_ws_doubles(const TkGeo& g) { return (size_t)g.m_np * TK_NMOM; }
RT_HD size_t tk_bwd_ws_floats(const TkGeo& g) { return (size_t)g.b_np * g.c4 * (2 + g.kc) * 4; }
RT_HD int tk_tri(int a, int b) { return TK_MAX_CIN + a * TK_MAX_CIN - a * (a - 1) / 2 + (b - a); }     // a <= b < 8

// ---------------------------------------------------------------------------------------------
// Input moments, in double from the first addition, about the pivot x0 = row 0 (d = x - x0: a constant column gives exact zeros and an
// off-centre cloud loses nothing to E[d d^T] - E[d] E[d]^T).
// 1: sh[j][tid] = the thread's sums over its rows (j < 44; entries beyond Cin are 0);  2: thread j < 44 adds the 64 lanes in ascending
// order -> part[wg][j].  LDS: sh [44][64] doubles.
template <int KC>
RT_HD void tk_mom_1(const TkGeo& g, int wg, int tid, double* sh) {
    double s1[KC], s2[KC * (KC + 1) / 2], x0[KC];
#pragma unroll
    for (int a = 0; a < KC; ++a) { s1[a] = 0.0; x0[a] = a < g.Cin ? (double)g.X[a] : 0.0; }
#pragma unroll
    for (int n = 0; n < KC * (KC + 1) / 2; ++n) s2[n] = 0.0;
    const long long r0 = (long long)wg * g.m_chunk, r1 = r0 + g.m_chunk < g.M ? r0 + g.m_chunk : g.M;
    for (long long r = r0 + tid; r < r1; r += TK_MOM_THREADS) {
        const float* p = g.X + r * g.ldx;
        double d[KC];
#pragma unroll
        for (int a = 0; a < KC; ++a) d[a] = a < g.Cin ? (double)p[a] - x0[a] : 0.0;
        int n = 0;
#pragma unroll
        for (int a = 0; a < KC; ++a) {
            s1[a] += d[a];
#pragma unroll
            for (int b = a; b < KC; ++b) s2[n++] += d[a] * d[b];
        }
    }
    for (int j = 0; j < TK_NMOM; ++j) sh[j * TK_MOM_THREADS + tid] = 0.0;
    int n = 0;
#pragma unroll
    for (int a = 0; a < KC; ++a) {
        sh[a * TK_MOM_THREADS + tid] = s1[a];
#pragma unroll
        for (int b = a; b < KC; ++b) sh[tk_tri(a, b) * TK_MOM_THREADS + tid] = s2[n++];
    }
}
RT_HD void tk_mom_2(const TkGeo& g, int wg, int tid, const double* sh, double* part) {
    if (tid >= TK_NMOM) return;
    double s = 0.0;
    for (int l = 0; l < TK_MOM_THREADS; ++l) s += sh[tid * TK_MOM_THREADS + l];
    part[(size_t)wg * TK_NMOM + tid] = s;
}
// The finaliser, one workgroup of 256.  1: thread j < 44: the chunks in ascending order -> sh[j];  2: thread t < 72: xmom = mu | Sigma;
// 3: per channel, mean_c = w_c mu + b_c, var_c = w_c^T Sigma w_c -> bn_save = scale | shift | mean | invstd and the running buffers
// (biased variance to normalise, unbiased for run_var).  LDS: sh [44] doubles.
RT_HD void tk_fin_1(const TkGeo& g, int tid, const double* part, double* sh) {
    if (tid >= TK_NMOM) return;
    double s = 0.0;
    for (int p = 0; p < g.m_np; ++p) s += part[(size_t)p * TK_NMOM + tid];
    sh[tid] = s;
}
RT_HD void tk_fin_2(const TkGeo& g, int tid, const double* sh, double* xmom) {
    if (tid >= TK_XMOM) return;
    const double inv = 1.0 / (double)g.M;
    if (tid < TK_MAX_CIN) {
        xmom[tid] = tid < g.Cin ? (double)g.X[tid] + sh[tid] * inv : 0.0;
        return;
    }
    const int a = (tid - TK_MAX_CIN) / TK_MAX_CIN, b = (tid - TK_MAX_CIN) % TK_MAX_CIN, lo = a < b ? a : b, hi = a < b ? b : a;
    xmom[tid] = sh[tk_tri(lo, hi)] * inv - (sh[lo] * inv) * (sh[hi] * inv);
}
RT_HD void tk_fin_3(const TkGeo& g, int tid, const double* xmom, float* bn_save, float* run_mean, float* run_var) {
    for (int c = tid; c < g.C; c += RT_THREADS) {
        const float* w = g.W + (size_t)c * g.Cin;
        double mean = g.bias ? (double)g.bias[c] : 0.0, var = 0.0;
        for (int a = 0; a < g.Cin; ++a) {
            mean += (double)w[a] * xmom[a];
            double row = 0.0;
            for (int b = 0; b < g.Cin; ++b) row += xmom[TK_MAX_CIN + a * TK_MAX_CIN + b] * (double)w[b];
            var += (double)w[a] * row;
        }
        if (var < 0.0) var = 0.0;                           // (a NaN stays a NaN)
        const double invstd = 1.0 / sqrt(var + (double)g.eps), scale = (double)g.gamma[c] * invstd;
        bn_save[c] = (float)scale;
        bn_save[g.C + c] = (float)((double)g.beta[c] - mean * scale);
        bn_save[2 * g.C + c] = (float)mean;
        bn_save[3 * g.C + c] = (float)invstd;
        if (run_mean) run_mean[c] = (float)((1.0 - (double)g.momentum) * run_mean[c] + (double)g.momentum * mean);
        if (run_var) run_var[c] = (float)((1.0 - (double)g.momentum) * run_var[c] + (double)g.momentum * var * ((double)g.M / (double)(g.M - 1)));
    }
}
// eval mode: bn_save from the running buffers, item c
RT_HD void tk_running_item(const TkGeo& g, int c, const float* run_mean, const float* run_var, float* bn_save) {
    if (c >= g.C) return;
    const double invstd = 1.0 / sqrt((double)run_var[c] + (double)g.eps), scale = (double)g.gamma[c] * invstd;
    bn_save[c] = (float)scale;
    bn_save[g.C + c] = (float)((double)g.beta[c] - (double)run_mean[c] * scale);
    bn_save[2 * g.C + c] = run_mean[c];
    bn_save[3 * g.C + c] = (float)invstd;
}

// ---------------------------------------------------------------------------------------------
// What a thread keeps of its 4 channels.  With xc = (x - mh) - ml (mu = mh + ml to fp64's digits in TK_MODE_BATCH, 0 otherwise) and
// t = w . xc:  u = t + bp,  z = u A + B (the activation's argument),  yhat = (u - mc) is.
//   batch:   A = gamma invstd, B = beta, bp = 0 (the bias cancels in the centred form), mc = 0, is = invstd
//   running: A = scale, B = shift, bp = bias, mc = running mean, is = invstd;   plain: A = 1, B = 0, bp = bias
// MODE is a template argument of everything that runs per row: the three variants differ in which pointers they read at all.
template <int KC>
struct TkCh { float w[4][KC], mh[KC], ml[KC]; rt_f4 A, B, bp, mc, is; };
template <int KC, int MODE>
RT_HD void tk_load_ch(const TkGeo& g, int cq, const float* bn_save, const double* xmom, TkCh<KC>& k) {
    const rt_f4 zero = rt_f4{0.f, 0.f, 0.f, 0.f}, one = rt_f4{1.f, 1.f, 1.f, 1.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int a = 0; a < KC; ++a) k.w[e][a] = a < g.Cin ? g.W[(size_t)(cq * 4 + e) * g.Cin + a] : 0.f;
#pragma unroll
    for (int a = 0; a < KC; ++a) {
        const double mu = MODE == TK_MODE_BATCH && a < g.Cin ? xmom[a] : 0.0;
        k.mh[a] = (float)mu;
        k.ml[a] = (float)(mu - (double)k.mh[a]);
    }
    const rt_f4 bias = g.bias ? rt_ld(g.bias + cq * 4) : zero;
    if (MODE == TK_MODE_BATCH) {
        k.A = rt_ld(bn_save + cq * 4); k.B = rt_ld(g.beta + cq * 4); k.bp = zero; k.mc = zero; k.is = rt_ld(bn_save + 3 * (size_t)g.C + cq * 4);
    } else if (MODE == TK_MODE_RUNNING) {
        k.A = rt_ld(bn_save + cq * 4); k.B = rt_ld(bn_save + (size_t)g.C + cq * 4); k.bp = bias;
        k.mc = rt_ld(bn_save + 2 * (size_t)g.C + cq * 4); k.is = rt_ld(bn_save + 3 * (size_t)g.C + cq * 4);
    } else {
        k.A = one; k.B = zero; k.bp = bias; k.mc = zero; k.is = zero;
    }
}
template <int KC>
RT_HD rt_f4 tk_u(const TkGeo& g, const TkCh<KC>& k, long long r, float (&xc)[KC]) {
    const float* p = g.X + r * g.ldx;
#pragma unroll
    for (int a = 0; a < KC; ++a) xc[a] = a < g.Cin ? (p[a] - k.mh[a]) - k.ml[a] : 0.f;
    rt_f4 u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float t = k.w[e][0] * xc[0];
#pragma unroll
        for (int a = 1; a < KC; ++a) t += k.w[e][a] * xc[a];
        u[e] = t + k.bp[e];
    }
    return u;
}
// GELU, the erf form of gelu_fwd_kernel: z Phi(z), Phi(z) = erfc(-z / sqrt 2) / 2;  derivative Phi(z) + z phi(z)
RT_HD float tk_cdf(float z) { return 0.5f * erfcf(-z * 0.70710678118654752440f); }
RT_HD float tk_act(float z, int act) {
    if (act == TK_ACT_RELU) return z < 0.f ? 0.f : z;
    if (act == TK_ACT_GELU) return z * tk_cdf(z);
    return z;
}
RT_HD float tk_dact(float z, int act) {
    if (act == TK_ACT_RELU) return z > 0.f ? 1.f : 0.f;
    if (act == TK_ACT_GELU) return fmaf(z * 0.39894228040143267794f, expf(-0.5f * z * z), tk_cdf(z));
    return 1.f;
}

// The apply pass: workgroup wg owns the rows [wg a_chunk, + a_chunk), thread (rl, tc) the quad cq0 + tc of every nrl-th of them.
template <int KC, int MODE>
RT_HD void tk_apply(const TkGeo& g, int wg, int cq0, int tid, const float* bn_save, const double* xmom, float* H) {
    const int tc = tid % g.ct, rl = tid / g.ct, cq = cq0 + tc;
    if (rl >= g.nrl || cq >= g.c4) return;
    TkCh<KC> k;
    tk_load_ch<KC, MODE>(g, cq, bn_save, xmom, k);
    const long long r0 = (long long)wg * g.a_chunk, r1 = r0 + g.a_chunk < g.M ? r0 + g.a_chunk : g.M;
    for (long long r = r0 + rl; r < r1; r += g.nrl) {
        float xc[KC];
        const rt_f4 u = tk_u<KC>(g, k, r, xc);
        rt_f4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = tk_act(u[e] * k.A[e] + k.B[e], g.act);
        rt_st(H + r * g.C + cq * 4, o);
    }
}

// ---------------------------------------------------------------------------------------------
// Backward sums per channel over the rows, y recomputed from X: dz = dH act'(z);  S0 = sum dz, S1 = sum dz yhat, S2[a] = sum dz xc[a].
// 1: sh[tid][2 + KC] quads = the thread's fp32 sums over its rows;  2: the row lanes in ascending order -> part[wg][cq][2 + KC] quads.
template <int KC, int MODE>
RT_HD void tk_bwd_1(const TkGeo& g, int wg, int cq0, int tid, const float* bn_save, const double* xmom, const float* dH, float* sh) {
    const int tc = tid % g.ct, rl = tid / g.ct, cq = cq0 + tc;
    if (rl >= g.nrl || cq >= g.c4) return;
    TkCh<KC> k;
    tk_load_ch<KC, MODE>(g, cq, bn_save, xmom, k);
    const rt_f4 zero = rt_f4{0.f, 0.f, 0.f, 0.f};
    rt_f4 s0 = zero, s1 = zero, s2[KC];
#pragma unroll
    for (int a = 0; a < KC; ++a) s2[a] = zero;
    const long long r0 = (long long)wg * g.b_chunk, r1 = r0 + g.b_chunk < g.M ? r0 + g.b_chunk : g.M;
    for (long long r = r0 + rl; r < r1; r += g.nrl) {
        float xc[KC];
        const rt_f4 u = tk_u<KC>(g, k, r, xc), d = rt_ld(dH + r * g.C + cq * 4);
        rt_f4 dz;
#pragma unroll
        for (int e = 0; e < 4; ++e) dz[e] = d[e] * tk_dact(u[e] * k.A[e] + k.B[e], g.act);
        s0 += dz;
        s1 += dz * ((u - k.mc) * k.is);
#pragma unroll
        for (int a = 0; a < KC; ++a) s2[a] += dz * xc[a];
    }
    float* dst = sh + (size_t)tid * (2 + KC) * 4;
    rt_st(dst, s0); rt_st(dst + 4, s1);
#pragma unroll
    for (int a = 0; a < KC; ++a) rt_st(dst + 8 + a * 4, s2[a]);
}
RT_HD void tk_bwd_2(const TkGeo& g, int wg, int cq0, int tid, const float* sh, float* part) {
    const int tc = tid % g.ct, rl = tid / g.ct, cq = cq0 + tc, nq = 2 + g.kc;
    if (rl != 0 || cq >= g.c4) return;
    float* dst = part + ((size_t)wg * g.c4 + cq) * nq * 4;
    for (int j = 0; j < nq; ++j) {
        rt_f4 s = rt_ld(sh + ((size_t)tid * nq + j) * 4);
        for (int q = 1; q < g.nrl; ++q) s += rt_ld(sh + ((size_t)(q * g.ct + tc) * nq + j) * 4);
        rt_st(dst + j * 4, s);
    }
}
RT_HD double tk_part_sum(const TkGeo& g, const float* part, int c, int j) {          // the chunks in ascending order, in double
    const int nq = 2 + g.kc;
    double s = 0.0;
    for (int p = 0; p < g.b_np; ++p) s += (double)part[(((size_t)p * g.c4 + c / 4) * nq + j) * 4 + c % 4];
    return s;
}
// item c.  batch: with dy_i = scale (dz_i - S0 / M - yhat_i S1 / M) and sum_i yhat_i (x_i - mu) = M invstd Sigma w_c,
//   dW_c = scale (S2 - S1 invstd Sigma w_c), db_c = 0 exactly, dgamma = S1, dbeta = S0;
// running: dW_c = scale S2, db_c = scale S0;   plain: dW_c = S2, db_c = S0.   db / dgamma / dbeta nullable.
RT_HD void tk_bwd_fin(const TkGeo& g, int c, const float* part, const float* bn_save, const double* xmom, float* dW, float* db, float* dgamma,
                      float* dbeta) {
    if (c >= g.C) return;
    const double S0 = tk_part_sum(g, part, c, 0), S1 = tk_part_sum(g, part, c, 1);
    const double scale = g.mode == TK_MODE_PLAIN ? 1.0 : (double)bn_save[c], invstd = g.mode == TK_MODE_PLAIN ? 0.0 : (double)bn_save[3 * (size_t)g.C + c];
    const float* w = g.W + (size_t)c * g.Cin;
    for (int a = 0; a < g.Cin; ++a) {
        double v = tk_part_sum(g, part, c, 2 + a);
        if (g.mode == TK_MODE_BATCH) {
            double row = 0.0;
            for (int b = 0; b < g.Cin; ++b) row += xmom[TK_MAX_CIN + a * TK_MAX_CIN + b] * (double)w[b];
            v -= S1 * invstd * row;
        }
        dW[(size_t)c * g.Cin + a] = (float)(scale * v);
    }
    if (db) db[c] = g.mode == TK_MODE_BATCH ? 0.f : (float)(scale * S0);
    if (g.mode != TK_MODE_PLAIN) {
        if (dgamma) dgamma[c] = (float)S1;
        if (dbeta) dbeta[c] = (float)S0;
    }
}

// ---------------------------------------------------------------------------------------------
// Token pooling.  y [B L][d]: out[b] = y[b L] | max_{1 <= l < L} y[b L + l], arg[b][c] = that l.  Strict comparison: the lowest row wins
// ties.  A NaN never displaces a number and a number displaces a NaN, so arg stays in [1, L): a NaN row inside an otherwise finite column
// is not selected, an all-NaN column takes row 1 and reports NaN.
// Workgroup (cloud b, quad block cq0); thread (rl, tc): 1: its rows 1 + rl, 1 + rl + nrl, ... -> sh_v / sh_a[tid] (arg 0: no row);
// 2: row lane 0 folds the lanes and writes both halves of out.  LDS: 256 value quads + 256 index quads.
struct TpGeo { int B, L, d, c4, ct, nrl, nqb; };          // nqb: quad blocks of ct per row
RT_HD bool tp_geo(int B, int L, int d, TpGeo& g) {
    if (B < 1 || L < 2 || d < 4 || d % 4 || d > (1 << 20) || L > (1 << 24) || (long long)B * L > (1LL << 30)) return false;
    g.B = B; g.L = L; g.d = d; g.c4 = d / 4;
    g.ct = g.c4 < RT_THREADS ? g.c4 : RT_THREADS;
    g.nrl = RT_THREADS / g.ct;
    g.nqb = (g.c4 + g.ct - 1) / g.ct;
    return (long long)B * g.nqb < (1LL << 31);
}
RT_HD bool tp_better(float v, int l, float best, int arg) {             // (v, l) replaces (best, arg)
    if (arg == 0) return true;
    return v > best || (best != best && v == v) || (v == best && l < arg) || (v != v && best != best && l < arg);
}
RT_HD void tp_fwd_1(const TpGeo& g, int b, int cq0, int tid, const float* y, float* sh_v, int* sh_a) {
    const int tc = tid % g.ct, rl = tid / g.ct, cq = cq0 + tc;
    if (rl >= g.nrl || cq >= g.c4) return;
    rt_f4 best = rt_f4{0.f, 0.f, 0.f, 0.f};
    tk_i4 arg = tk_i4{0, 0, 0, 0};
    for (int l = 1 + rl; l < g.L; l += g.nrl) {
        const rt_f4 v = rt_ld(y + ((long long)b * g.L + l) * g.d + cq * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (tp_better(v[e], l, best[e], arg[e])) { best[e] = v[e]; arg[e] = l; }
    }
    rt_st(sh_v + (size_t)tid * 4, best);
    *(tk_i4*)(sh_a + (size_t)tid * 4) = arg;
}
RT_HD void tp_fwd_2(const TpGeo& g, int b, int cq0, int tid, const float* y, const float* sh_v, const int* sh_a, float* out, int* arg) {
    const int tc = tid % g.ct, rl = tid / g.ct, cq = cq0 + tc;
    if (rl != 0 || cq >= g.c4) return;
    rt_f4 best = rt_ld(sh_v + (size_t)tid * 4);
    tk_i4 a = *(const tk_i4*)(sh_a + (size_t)tid * 4);    // (row lane 0 always has row 1)
    for (int q = 1; q < g.nrl; ++q) {
        const rt_f4 v = rt_ld(sh_v + (size_t)(q * g.ct + tc) * 4);
        const tk_i4 l = *(const tk_i4*)(sh_a + (size_t)(q * g.ct + tc) * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (l[e] != 0 && tp_better(v[e], l[e], best[e], a[e])) { best[e] = v[e]; a[e] = l[e]; }
    }
    float* o = out + (size_t)b * 2 * g.d;
    rt_st(o + cq * 4, rt_ld(y + (long long)b * g.L * g.d + cq * 4));
    rt_st(o + g.d + cq * 4, best);
    *(tk_i4*)(arg + (size_t)b * g.d + cq * 4) = a;
}
// dy[r][c]: row 0 of a cloud = the cls half of dOut, row arg = the max half, 0 elsewhere.  Item (row r of B L, quad cq): one writer each.
RT_HD void tp_bwd_item(const TpGeo& g, long long r, int cq, const float* dOut, const int* arg, float* dy) {
    const long long b = r / g.L;
    const int l = (int)(r - b * g.L);
    rt_f4 o;
    if (l == 0) {
        o = rt_ld(dOut + b * 2 * g.d + cq * 4);
    } else {
        const rt_f4 m = rt_ld(dOut + b * 2 * g.d + g.d + cq * 4);
        const tk_i4 a = *(const tk_i4*)(arg + b * g.d + cq * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = a[e] == l ? m[e] : 0.f;
    }
    rt_st(dy + r * g.d + cq * 4, o);
}
