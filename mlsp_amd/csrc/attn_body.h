// The bodies of the kernels of attn.hip, one function per phase between two workgroup barriers, each a function of (workgroup, thread):
// attn.hip calls them with blockIdx / threadIdx and a __syncthreads() between phases, tools/attn_host_check/main.hip calls them on the
// host, one call per work-item and phase, against exact-size heap buffers (no lane talks to another inside a phase: what crosses lanes
// goes through LDS and a barrier, so the host walk computes what the GPU computes).  Element offsets into global memory are 64-bit.
#pragma once
#include <math.h>
#include <stddef.h>
#include "rowtile.h"

#define AB_WAVES 4
#define AB_LDS_MAX (160 * 1024)
#define AB_MAX_DH 128
#define AB_MAX_L 512
#define AB_MAX_LDH 16384

// ---------------------------------------------------------------------------------------------
// Multi-head attention core.  qkv [B L][ld]: q, k, v of head h in columns h dh, d + h dh, 2 d + h dh (d = H dh); out / dout [B L][d];
// lse [B][H][L]; dqkv [B L][ldd] laid out as qkv.  A workgroup is (b, h, block of qb rows); wave w of it owns rows q0 + w, q0 + w + 4, ..
// (the backward takes one block per (b, h), qb >= L: its column phase needs delta_i of every row, which its row phase leaves in LDS)
// LDS (floats): A0 [L][kst] | A1 [L][kst] | S [4][lp] | E [4][lp] | vec [4][2 dh] | lse_s [lp] | del_s [lp]
struct MhsaGeo {
    int B, L, H, dh, ld, ldd, qb, nqb, kst, lp;
    float scale;
};
RT_HD size_t mhsa_lds_floats(const MhsaGeo& g) { return (size_t)2 * g.L * g.kst + (size_t)AB_WAVES * 2 * g.lp + (size_t)AB_WAVES * 2 * g.dh + (size_t)2 * g.lp; }
// the geometry of a shape, or false outside the limits: dh % 4 == 0, dh <= 128, L <= 512, L dh <= 16384 (two [L][dh] arrays in LDS)
RT_HD bool mhsa_geo(int B, int L, int H, int dh, int ld, int ldd, float scale, bool whole_head, MhsaGeo& g) {
    if (B <= 0 || L <= 0 || H <= 0 || dh <= 0 || dh % 4 || dh > AB_MAX_DH || L > AB_MAX_L || (long long)L * dh > AB_MAX_LDH) return false;
    const long long d = (long long)H * dh;
    if (3 * d > ld || 3 * d > ldd || ld % 4 || ldd % 4 || (long long)B * L > (1LL << 30)) return false;
    g.B = B; g.L = L; g.H = H; g.dh = dh; g.ld = ld; g.ldd = ldd; g.scale = scale;
    int qb = whole_head ? L : (L + 7) / 8;
    qb = (qb + AB_WAVES - 1) / AB_WAVES * AB_WAVES;
    g.qb = qb < 16 ? 16 : qb;
    g.nqb = (L + g.qb - 1) / g.qb;
    g.lp = (L + 3) / 4 * 4;
    g.kst = dh + 4;                                        // rows 16 bytes apart in the banks: a wave's 128-bit reads of 64 rows do not collide
    if (mhsa_lds_floats(g) * sizeof(float) > AB_LDS_MAX) g.kst = dh;
    if (mhsa_lds_floats(g) * sizeof(float) > AB_LDS_MAX) return false;
    return (long long)B * H * g.nqb < (1LL << 31);
}
struct MhsaLds { float *A0, *A1, *S, *E, *vec, *lse_s, *del_s; };
RT_HD MhsaLds mhsa_lds(const MhsaGeo& g, float* lds, int w) {
    MhsaLds m;
    m.A0 = lds; m.A1 = m.A0 + (size_t)g.L * g.kst;
    float* s = m.A1 + (size_t)g.L * g.kst;
    m.S = s + w * g.lp; m.E = s + (AB_WAVES + w) * g.lp;
    float* v = s + 2 * AB_WAVES * g.lp;
    m.vec = v + w * 2 * g.dh;
    m.lse_s = v + AB_WAVES * 2 * g.dh; m.del_s = m.lse_s + g.lp;
    return m;
}
struct MhsaWho { int b, h, q0, q1; long long row0; };      // rows [q0, q1) of cloud b; row0 = b L
RT_HD MhsaWho mhsa_who(const MhsaGeo& g, int bid) {
    MhsaWho o;
    const int qblk = bid % g.nqb, bh = bid / g.nqb;
    o.h = bh % g.H; o.b = bh / g.H;
    o.q0 = qblk * g.qb; o.q1 = o.q0 + g.qb < g.L ? o.q0 + g.qb : g.L;
    o.row0 = (long long)o.b * g.L;
    return o;
}
RT_HD int mhsa_steps(const MhsaGeo& g) { return g.qb / AB_WAVES; }
// sum_c a[c] b[c], ascending c, one fma per term (the same bits whichever operand sits in `a`)
RT_HD float mhsa_dot(const float* a, const float* b, int dh) {
    float acc = 0.f;
    for (int c = 0; c < dh; c += 4) {
        const rt_f4 x = rt_ld(a + c), y = rt_ld(b + c);
        acc = fmaf(x.x, y.x, acc); acc = fmaf(x.y, y.y, acc); acc = fmaf(x.z, y.z, acc); acc = fmaf(x.w, y.w, acc);
    }
    return acc;
}
// A0 / A1 <- the [L][dh] column slices of X / Y at columns cx / cy (every row of the cloud)
RT_HD void mhsa_stage(const MhsaGeo& g, const MhsaWho& o, int tid, const float* X, int ldx, int cx, const float* Y, int ldy, int cy, float* lds) {
    const MhsaLds m = mhsa_lds(g, lds, 0);
    const int dh4 = g.dh / 4;
    for (int it = tid; it < g.L * dh4; it += RT_THREADS) {
        const int j = it / dh4, cq = it - j * dh4;
        rt_st(m.A0 + (size_t)j * g.kst + cq * 4, rt_ld(X + (o.row0 + j) * ldx + cx + cq * 4));
        rt_st(m.A1 + (size_t)j * g.kst + cq * 4, rt_ld(Y + (o.row0 + j) * ldy + cy + cq * 4));
    }
}
// vec[w][slot] <- dh floats of row i of X at column cx
RT_HD void mhsa_vec_load(const MhsaGeo& g, const MhsaWho& o, int lane, int i, const float* X, int ldx, int cx, float* dst) {
    if (lane < g.dh / 4) rt_st(dst + lane * 4, rt_ld(X + (o.row0 + i) * ldx + cx + lane * 4));
}

// forward, row step r.  a: q_i -> vec;  b: S[j] = scale q_i.k_j;  c: E[j] = exp(S[j] - max S);  d: out_i = sum_j E[j] v_j / sum_j E[j], lse
RT_HD void mhsa_fwd_a(const MhsaGeo& g, int bid, int tid, int r, const float* qkv, float* lds) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, i = o.q0 + r * AB_WAVES + w;
    if (i >= o.q1) return;
    mhsa_vec_load(g, o, lane, i, qkv, g.ld, o.h * g.dh, mhsa_lds(g, lds, w).vec);
}
RT_HD void mhsa_fwd_b(const MhsaGeo& g, int bid, int tid, int r, float* lds) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, i = o.q0 + r * AB_WAVES + w;
    if (i >= o.q1) return;
    const MhsaLds m = mhsa_lds(g, lds, w);
    for (int j = lane; j < g.L; j += 64) m.S[j] = mhsa_dot(m.vec, m.A0 + (size_t)j * g.kst, g.dh) * g.scale;
}
RT_HD float mhsa_row_max(const float* S, int L) {
    float mx = S[0];
    for (int j = 1; j < L; ++j) mx = fmaxf(mx, S[j]);
    return mx;
}
RT_HD void mhsa_fwd_c(const MhsaGeo& g, int bid, int tid, int r, float* lds) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, i = o.q0 + r * AB_WAVES + w;
    if (i >= o.q1) return;
    const MhsaLds m = mhsa_lds(g, lds, w);
    const float mx = mhsa_row_max(m.S, g.L);
    for (int j = lane; j < g.L; j += 64) m.E[j] = expf(m.S[j] - mx);
}
RT_HD void mhsa_fwd_d(const MhsaGeo& g, int bid, int tid, int r, float* lds, float* out, float* lse) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, i = o.q0 + r * AB_WAVES + w;
    if (i >= o.q1) return;
    const MhsaLds m = mhsa_lds(g, lds, w);
    const int c0 = lane < g.dh ? lane : 0, c1 = lane + 64 < g.dh ? lane + 64 : c0;
    float l = 0.f, a0 = 0.f, a1 = 0.f;
    for (int j = 0; j < g.L; ++j) {
        const float e = m.E[j];
        const float* v = m.A1 + (size_t)j * g.kst;
        l += e;
        a0 = fmaf(e, v[c0], a0); a1 = fmaf(e, v[c1], a1);
    }
    float* dst = out + (o.row0 + i) * ((long long)g.H * g.dh) + o.h * g.dh;
    if (lane < g.dh) dst[lane] = a0 / l;
    if (lane + 64 < g.dh) dst[lane + 64] = a1 / l;
    if (lane == 0) lse[((long long)o.b * g.H + o.h) * g.L + i] = mhsa_row_max(m.S, g.L) + logf(l);
}

// backward, rows (A0 = K, A1 = V).  a: q_i | dout_i -> vec;  b: S[j] = P_ij = exp(scale q_i.k_j - lse_i), E[j] = dP_ij = dout_i.v_j;
// d: delta_i = sum_j P_ij dP_ij / sum_j P_ij (= dout_i.out_i in exact arithmetic; formed from the very P and dP it is subtracted from, so
// that sum_j dS_ij carries only their rounding -- the sum that the key bias gradient, exactly 0, is made of), del_s[i] <- delta_i,
// dq_i = scale sum_j dS_ij k_j, dS_ij = P_ij (dP_ij - delta_i)
RT_HD void mhsa_bwd_row_a(const MhsaGeo& g, int bid, int tid, int r, const float* qkv, const float* dout, float* lds) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, i = o.q0 + r * AB_WAVES + w;
    if (i >= o.q1) return;
    float* vec = mhsa_lds(g, lds, w).vec;
    const int d = g.H * g.dh;
    mhsa_vec_load(g, o, lane, i, qkv, g.ld, o.h * g.dh, vec);
    mhsa_vec_load(g, o, lane, i, dout, d, o.h * g.dh, vec + g.dh);
}
RT_HD void mhsa_bwd_row_b(const MhsaGeo& g, int bid, int tid, int r, const float* lse, float* lds) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, i = o.q0 + r * AB_WAVES + w;
    if (i >= o.q1) return;
    const MhsaLds m = mhsa_lds(g, lds, w);
    const float li = lse[((long long)o.b * g.H + o.h) * g.L + i];
    for (int j = lane; j < g.L; j += 64) {
        m.S[j] = expf(mhsa_dot(m.vec, m.A0 + (size_t)j * g.kst, g.dh) * g.scale - li);
        m.E[j] = mhsa_dot(m.vec + g.dh, m.A1 + (size_t)j * g.kst, g.dh);
    }
}
// sum_j P[j] dP[j] / sum_j P[j], both sums in fp64 in ascending j (the same in every lane).  P is recomputed from the fp32 lse, so its row sum
// is 1 only to an ulp of lse; dividing by it makes sum_j P[j] (dP[j] - delta) vanish to the rounding of its terms.
RT_HD float mhsa_delta(const float* P, const float* dP, int L) {
    double t = 0.0, n = 0.0;
    for (int j = 0; j < L; ++j) { t = fma((double)P[j], (double)dP[j], t); n += (double)P[j]; }
    return (float)(t / n);
}
RT_HD void mhsa_bwd_row_d(const MhsaGeo& g, int bid, int tid, int r, float* lds, float* dqkv) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, i = o.q0 + r * AB_WAVES + w;
    if (i >= o.q1) return;
    const MhsaLds m = mhsa_lds(g, lds, w);
    const int c0 = lane < g.dh ? lane : 0, c1 = lane + 64 < g.dh ? lane + 64 : c0;
    const float delta = mhsa_delta(m.S, m.E, g.L);
    if (lane == 0) m.del_s[i] = delta;
    float a0 = 0.f, a1 = 0.f;
    for (int j = 0; j < g.L; ++j) {
        const float s = m.S[j] * (m.E[j] - delta);
        const float* k = m.A0 + (size_t)j * g.kst;
        a0 = fmaf(s, k[c0], a0); a1 = fmaf(s, k[c1], a1);
    }
    float* dst = dqkv + (o.row0 + i) * g.ldd + o.h * g.dh;
    if (lane < g.dh) dst[lane] = a0 * g.scale;
    if (lane + 64 < g.dh) dst[lane + 64] = a1 * g.scale;
}
// backward, columns (A0 = Q, A1 = dout, both staged by mhsa_stage).  stats: lse_s[i] for every row of the cloud (del_s: the row phase);
// a: k_j | v_j -> vec;  b: S[i] = P_ij, E[i] = dS_ij;  d: dk_j = scale sum_i dS_ij q_i, dv_j = sum_i P_ij dout_i
RT_HD void mhsa_bwd_col_stats(const MhsaGeo& g, int bid, int tid, const float* lse, float* lds) {
    const MhsaWho o = mhsa_who(g, bid);
    const MhsaLds m = mhsa_lds(g, lds, 0);
    for (int i = tid; i < g.L; i += RT_THREADS) m.lse_s[i] = lse[((long long)o.b * g.H + o.h) * g.L + i];
}
RT_HD void mhsa_bwd_col_a(const MhsaGeo& g, int bid, int tid, int r, const float* qkv, float* lds) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, j = o.q0 + r * AB_WAVES + w;
    if (j >= o.q1) return;
    float* vec = mhsa_lds(g, lds, w).vec;
    const int d = g.H * g.dh;
    mhsa_vec_load(g, o, lane, j, qkv, g.ld, d + o.h * g.dh, vec);
    mhsa_vec_load(g, o, lane, j, qkv, g.ld, 2 * d + o.h * g.dh, vec + g.dh);
}
RT_HD void mhsa_bwd_col_b(const MhsaGeo& g, int bid, int tid, int r, float* lds) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, j = o.q0 + r * AB_WAVES + w;
    if (j >= o.q1) return;
    const MhsaLds m = mhsa_lds(g, lds, w);
    for (int i = lane; i < g.L; i += 64) {
        const float p = expf(mhsa_dot(m.A0 + (size_t)i * g.kst, m.vec, g.dh) * g.scale - m.lse_s[i]);
        m.S[i] = p;
        m.E[i] = p * (mhsa_dot(m.A1 + (size_t)i * g.kst, m.vec + g.dh, g.dh) - m.del_s[i]);
    }
}
RT_HD void mhsa_bwd_col_d(const MhsaGeo& g, int bid, int tid, int r, float* lds, float* dqkv) {
    const MhsaWho o = mhsa_who(g, bid);
    const int w = tid >> 6, lane = tid & 63, j = o.q0 + r * AB_WAVES + w;
    if (j >= o.q1) return;
    const MhsaLds m = mhsa_lds(g, lds, w);
    const int c0 = lane < g.dh ? lane : 0, c1 = lane + 64 < g.dh ? lane + 64 : c0, d = g.H * g.dh;
    float k0 = 0.f, k1 = 0.f, v0 = 0.f, v1 = 0.f;
    for (int i = 0; i < g.L; ++i) {
        const float ds = m.E[i], p = m.S[i];
        const float* q = m.A0 + (size_t)i * g.kst;
        const float* go = m.A1 + (size_t)i * g.kst;
        k0 = fmaf(ds, q[c0], k0); k1 = fmaf(ds, q[c1], k1);
        v0 = fmaf(p, go[c0], v0); v1 = fmaf(p, go[c1], v1);
    }
    float* dst = dqkv + (o.row0 + j) * g.ldd + o.h * g.dh;
    if (lane < g.dh) { dst[d + lane] = k0 * g.scale; dst[2 * d + lane] = v0; }
    if (lane + 64 < g.dh) { dst[d + lane + 64] = k1 * g.scale; dst[2 * d + lane + 64] = v1; }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm over the d channels of a row, a wave per row (rows row0 .. row0 + 3 of a workgroup step); u = x + s[row / rps] a.
// LDS: red [4][64] | red2 [4][64].
struct LnGeo {
    long long rows; int d4, rps; float eps;
    const float *x, *a, *s, *gamma, *beta;
};
RT_HD rt_f4 ln_u(const LnGeo& g, long long row, int q) {
    rt_f4 u = rt_ld(g.x + (row * g.d4 + q) * 4);
    if (g.a) {
        const rt_f4 a = rt_ld(g.a + (row * g.d4 + q) * 4);
        u = g.s ? u + g.s[row / g.rps] * a : u + a;
    }
    return u;
}
RT_HD float ln_sum64(const float* red) {
    float t = 0.f;
    for (int l = 0; l < 64; ++l) t += red[l];
    return t;
}
// 1: U <- u (U nullable), red <- the lanes' sums of u;  2: red2 <- the lanes' sums of (u - mean)^2;  3: y, mean, rstd
RT_HD void ln_fwd_1(const LnGeo& g, long long row0, int tid, float* U, float* lds) {
    const int w = tid >> 6, lane = tid & 63;
    const long long row = row0 + w;
    if (row >= g.rows) return;
    float t = 0.f;
    for (int q = lane; q < g.d4; q += 64) {
        const rt_f4 u = ln_u(g, row, q);
        if (U) rt_st(U + (row * g.d4 + q) * 4, u);
        t += (u.x + u.y) + (u.z + u.w);
    }
    lds[w * 64 + lane] = t;
}
RT_HD void ln_fwd_2(const LnGeo& g, long long row0, int tid, float* lds) {
    const int w = tid >> 6, lane = tid & 63;
    const long long row = row0 + w;
    if (row >= g.rows) return;
    const float mean = ln_sum64(lds + w * 64) / (float)(g.d4 * 4);
    float t = 0.f;
    for (int q = lane; q < g.d4; q += 64) {
        const rt_f4 c = ln_u(g, row, q) - mean;
        t += (c.x * c.x + c.y * c.y) + (c.z * c.z + c.w * c.w);
    }
    lds[(AB_WAVES + w) * 64 + lane] = t;
}
RT_HD void ln_fwd_3(const LnGeo& g, long long row0, int tid, float* lds, float* Y, float* mean_out, float* rstd_out) {
    const int w = tid >> 6, lane = tid & 63;
    const long long row = row0 + w;
    if (row >= g.rows) return;
    const float mean = ln_sum64(lds + w * 64) / (float)(g.d4 * 4);
    const float rstd = 1.0f / sqrtf(ln_sum64(lds + (AB_WAVES + w) * 64) / (float)(g.d4 * 4) + g.eps);
    if (lane == 0) { mean_out[row] = mean; rstd_out[row] = rstd; }
    for (int q = lane; q < g.d4; q += 64)
        rt_st(Y + (row * g.d4 + q) * 4, (ln_u(g, row, q) - mean) * rstd * rt_ld(g.gamma + q * 4) + rt_ld(g.beta + q * 4));
}
// backward of a row: t = rstd (g - mean(g) - xhat mean(g xhat)) + du, g = dy gamma, xhat = (u - mean) rstd;  dx <- t, da <- s t.
// dy NULL (the residual add alone): t = du, only da is written.  u: the saved sum (LnGeo.x, with a = NULL).
struct LnBwd { const float *dy, *du, *mean, *rstd; float *dx, *da; };
RT_HD void ln_bwd_1(const LnGeo& g, const LnBwd& b, long long row0, int tid, float* lds) {
    const int w = tid >> 6, lane = tid & 63;
    const long long row = row0 + w;
    if (row >= g.rows || !b.dy) return;
    const float mean = b.mean[row], rstd = b.rstd[row];
    float t1 = 0.f, t2 = 0.f;
    for (int q = lane; q < g.d4; q += 64) {
        const rt_f4 xh = (rt_ld(g.x + (row * g.d4 + q) * 4) - mean) * rstd, gg = rt_ld(b.dy + (row * g.d4 + q) * 4) * rt_ld(g.gamma + q * 4);
        const rt_f4 gx = gg * xh;
        t1 += (gg.x + gg.y) + (gg.z + gg.w);
        t2 += (gx.x + gx.y) + (gx.z + gx.w);
    }
    lds[w * 64 + lane] = t1;
    lds[(AB_WAVES + w) * 64 + lane] = t2;
}
RT_HD void ln_bwd_2(const LnGeo& g, const LnBwd& b, long long row0, int tid, float* lds) {
    const int w = tid >> 6, lane = tid & 63;
    const long long row = row0 + w;
    if (row >= g.rows) return;
    const float sc = g.s ? g.s[row / g.rps] : 1.f;
    float mean = 0.f, rstd = 0.f, m1 = 0.f, m2 = 0.f;
    if (b.dy) {
        mean = b.mean[row]; rstd = b.rstd[row];
        m1 = ln_sum64(lds + w * 64) / (float)(g.d4 * 4);
        m2 = ln_sum64(lds + (AB_WAVES + w) * 64) / (float)(g.d4 * 4);
    }
    for (int q = lane; q < g.d4; q += 64) {
        const long long at = (row * g.d4 + q) * 4;
        rt_f4 t = rt_f4{0.f, 0.f, 0.f, 0.f};
        if (b.dy) {
            const rt_f4 xh = (rt_ld(g.x + at) - mean) * rstd, gg = rt_ld(b.dy + at) * rt_ld(g.gamma + q * 4);
            t = ((gg - m1) - xh * m2) * rstd;
        }
        if (b.du) t = t + rt_ld(b.du + at);
        if (b.dx) rt_st(b.dx + at, t);
        if (b.da) rt_st(b.da + at, t * sc);
    }
}
// dgamma / dbeta partials of the rows [e0, e1): threads are (row lane r < rl, channel quad tc < ct); part[g][cq] = {dgamma quad, dbeta quad}.
// LDS: sh [256][2] quads.
RT_HD void ln_par_1(const LnGeo& g, const LnBwd& b, long long e0, long long e1, int cq0, int ct, int rl, int tid, float* lds) {
    const int tc = tid % ct, r = tid / ct, cq = cq0 + tc;
    rt_f4 ag = rt_f4{0.f, 0.f, 0.f, 0.f}, ab = rt_f4{0.f, 0.f, 0.f, 0.f};
    if (r < rl && cq < g.d4)
        for (long long e = e0 + r; e < e1; e += rl) {
            const rt_f4 dy = rt_ld(b.dy + (e * g.d4 + cq) * 4);
            ag += dy * ((rt_ld(g.x + (e * g.d4 + cq) * 4) - b.mean[e]) * b.rstd[e]);
            ab += dy;
        }
    rt_st(lds + (size_t)tid * 8, ag);
    rt_st(lds + (size_t)tid * 8 + 4, ab);
}
RT_HD void ln_par_2(const LnGeo& g, int bid, int cq0, int ct, int rl, int tid, const float* lds, float* part) {
    const int tc = tid % ct, r = tid / ct, cq = cq0 + tc;
    if (r != 0 || cq >= g.d4) return;
    rt_f4 ag = rt_ld(lds + (size_t)tid * 8), ab = rt_ld(lds + (size_t)tid * 8 + 4);
    for (int q = 1; q < rl; ++q) {
        ag += rt_ld(lds + (size_t)(q * ct + tc) * 8);
        ab += rt_ld(lds + (size_t)(q * ct + tc) * 8 + 4);
    }
    rt_st(part + ((size_t)bid * g.d4 + cq) * 8, ag);
    rt_st(part + ((size_t)bid * g.d4 + cq) * 8 + 4, ab);
}
RT_HD void ln_par_fin(const float* part, int nparts, int d, int c, float* dgamma, float* dbeta) {
    if (c >= d) return;
    double sg = 0.0, sb = 0.0;
    for (int p = 0; p < nparts; ++p) {
        const float* q = part + ((size_t)p * (d / 4) + c / 4) * 8;
        sg += q[c % 4]; sb += q[4 + c % 4];
    }
    dgamma[c] = (float)sg; dbeta[c] = (float)sb;
}

// ---------------------------------------------------------------------------------------------
// GELU, the erf form: y = x Phi(x), Phi(x) = erfc(-x / sqrt 2) / 2 (erfc keeps the negative tail's digits);  dx = dy (Phi(x) + x phi(x))
RT_HD float gelu_phi_cdf(float x) { return 0.5f * erfcf(-x * 0.70710678118654752440f); }
RT_HD void gelu_fwd_quad(const float* x, long long t, float* y) {
    rt_f4 a = rt_ld(x + t * 4);
    a.x *= gelu_phi_cdf(a.x); a.y *= gelu_phi_cdf(a.y); a.z *= gelu_phi_cdf(a.z); a.w *= gelu_phi_cdf(a.w);
    rt_st(y + t * 4, a);
}
RT_HD float gelu_grad(float x) { return fmaf(x * 0.39894228040143267794f, expf(-0.5f * x * x), gelu_phi_cdf(x)); }
RT_HD void gelu_bwd_quad(const float* dy, const float* x, long long t, float* dx) {
    const rt_f4 g = rt_ld(dy + t * 4), a = rt_ld(x + t * 4);
    rt_st(dx + t * 4, rt_f4{g.x * gelu_grad(a.x), g.y * gelu_grad(a.y), g.z * gelu_grad(a.z), g.w * gelu_grad(a.w)});
}
