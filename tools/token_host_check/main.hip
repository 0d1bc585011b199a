// Host sanitizer check of the kernels of csrc/token.hip: their bodies (csrc/token_body.h, one function per phase between two barriers) run
// on the host, one call per work-item and phase in the order token.hip runs them, against heap buffers of exactly the sizes the Python
// layer allocates (functional._ThinIn, _TokenPool) and "LDS" / workspace heap blocks of exactly the bytes the launches use -- an index
// past either end of anything is an AddressSanitizer report.  The results are also compared with a plain double-precision loop.
// A stand-alone program that needs no GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/token_host_check/main.hip -o build/token_host_check && build/token_host_check
#include <hip/hip_runtime.h>
#include "../../mlsp_amd/csrc/token_body.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fails = 0;
static double worst_all = 0.0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// exact-size, 16-byte-aligned heap array
template <typename T>
struct Buf {
    T* p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (posix_memalign((void**)&p, 16, (n ? n : 1) * sizeof(T))) abort(); for (size_t i = 0; i < n; ++i) p[i] = T(0); }
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
};
static uint32_t rng_state = 2463534242u;
static uint32_t rnd_u() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd() { return (float)(rnd_u() & 0xffff) / 32768.0f - 1.0f; }
static void fill(Buf<float>& b, float amp, float off = 0.f) { for (size_t i = 0; i < b.n; ++i) b.p[i] = off + rnd() * amp; }
// max |got - want| / max(max |want|, floor)
static double worst(const float* got, const std::vector<double>& want, double floor = 0.0) {
    double e = 0.0, m = 1e-30 + floor;
    for (size_t i = 0; i < want.size(); ++i) { e = fmax(e, fabs((double)got[i] - want[i])); m = fmax(m, fabs(want[i])); }
    return e / m;
}
static double act_d(double z, int act) { return act == TK_ACT_RELU ? (z > 0 ? z : 0.0) : act == TK_ACT_GELU ? z * 0.5 * erfc(-z / sqrt(2.0)) : z; }
static double dact_d(double z, int act) {
    return act == TK_ACT_RELU ? (z > 0 ? 1.0 : 0.0) : act == TK_ACT_GELU ? 0.5 * erfc(-z / sqrt(2.0)) + z * exp(-0.5 * z * z) / sqrt(2.0 * M_PI) : 1.0;
}

template <int KC, int MODE>
static void thin_run(const TkGeo& g, Buf<float>& H, Buf<float>& bn_save, Buf<double>& xmom, Buf<float>& rm, Buf<float>& rv, Buf<float>& dH,
                     Buf<float>& dW, Buf<float>& db, Buf<float>& dgamma, Buf<float>& dbeta) {
    // forward: thin_in_moments_kernel, thin_in_finalize_kernel | thin_in_running_kernel, thin_in_apply_kernel
    if (g.mode == TK_MODE_BATCH) {
        Buf<double> part(tk_fwd_ws_doubles(g)), sh(TK_NMOM * TK_MOM_THREADS), shf(TK_NMOM);
        for (int wg = 0; wg < g.m_np; ++wg) {
            for (int tid = 0; tid < TK_MOM_THREADS; ++tid) tk_mom_1<KC>(g, wg, tid, sh.p);
            for (int tid = 0; tid < TK_MOM_THREADS; ++tid) tk_mom_2(g, wg, tid, sh.p, part.p);
        }
        for (int tid = 0; tid < RT_THREADS; ++tid) tk_fin_1(g, tid, part.p, shf.p);
        for (int tid = 0; tid < RT_THREADS; ++tid) tk_fin_2(g, tid, shf.p, xmom.p);
        for (int tid = 0; tid < RT_THREADS; ++tid) tk_fin_3(g, tid, xmom.p, bn_save.p, rm.p, rv.p);
    } else if (g.mode == TK_MODE_RUNNING) {
        for (int c = 0; c < (g.C + RT_THREADS - 1) / RT_THREADS * RT_THREADS; ++c) tk_running_item(g, c, rm.p, rv.p, bn_save.p);
    }
    const float* bs = g.mode == TK_MODE_PLAIN ? nullptr : bn_save.p;
    const double* xm = g.mode == TK_MODE_BATCH ? xmom.p : nullptr;
    for (int wg = 0; wg < g.a_np; ++wg)
        for (int cq0 = 0; cq0 < g.c4; cq0 += g.ct)
            for (int tid = 0; tid < RT_THREADS; ++tid) tk_apply<KC, MODE>(g, wg, cq0, tid, bs, xm, H.p);
    // backward: thin_in_bwd_sums_kernel, thin_in_bwd_finalize_kernel
    Buf<float> part(tk_bwd_ws_floats(g)), sh((size_t)RT_THREADS * (2 + KC) * 4);
    for (int wg = 0; wg < g.b_np; ++wg)
        for (int cq0 = 0; cq0 < g.c4; cq0 += g.ct) {
            for (int tid = 0; tid < RT_THREADS; ++tid) tk_bwd_1<KC, MODE>(g, wg, cq0, tid, bs, xm, dH.p, sh.p);
            for (int tid = 0; tid < RT_THREADS; ++tid) tk_bwd_2(g, wg, cq0, tid, sh.p, part.p);
        }
    for (int c = 0; c < (g.C + RT_THREADS - 1) / RT_THREADS * RT_THREADS; ++c)
        tk_bwd_fin(g, c, part.p, bs, xm, dW.p, db.p, g.mode == TK_MODE_PLAIN ? nullptr : dgamma.p, g.mode == TK_MODE_PLAIN ? nullptr : dbeta.p);
}

static void thin_case(int M, int Cin, int C, int mode, int act, float off) {
    const float eps = 1e-5f, mom = 0.1f;
    TkGeo g;
    EXPECT(tk_geo(M, Cin, C, Cin, act, mode, eps, mom, g));
    Buf<float> X((size_t)M * Cin), W((size_t)C * Cin), bias(C), gamma(C), beta(C), rm(C), rv(C), H((size_t)M * C), bn_save(4 * (size_t)C), dH((size_t)M * C),
        dW((size_t)C * Cin), db(C), dgamma(C), dbeta(C);
    Buf<double> xmom(TK_XMOM);
    fill(X, 1.f, off); fill(W, 1.f); fill(bias, 0.5f); fill(gamma, 1.f); fill(beta, 0.5f); fill(rm, 0.5f); fill(dH, 1.f);
    for (int c = 0; c < C; ++c) rv.p[c] = 0.5f + fabsf(rnd());
    gamma.p[1] = 0.f;
    std::vector<double> rm0(rm.p, rm.p + C), rv0(rv.p, rv.p + C);
    g.X = X.p; g.W = W.p; g.bias = bias.p;
    if (mode != TK_MODE_PLAIN) { g.gamma = gamma.p; g.beta = beta.p; }
#define RUN(KC_, MODE_) thin_run<KC_, MODE_>(g, H, bn_save, xmom, rm, rv, dH, dW, db, dgamma, dbeta)
    if (g.kc == 4) { if (mode == TK_MODE_BATCH) RUN(4, TK_MODE_BATCH); else if (mode == TK_MODE_RUNNING) RUN(4, TK_MODE_RUNNING); else RUN(4, TK_MODE_PLAIN); }
    else { if (mode == TK_MODE_BATCH) RUN(8, TK_MODE_BATCH); else if (mode == TK_MODE_RUNNING) RUN(8, TK_MODE_RUNNING); else RUN(8, TK_MODE_PLAIN); }
#undef RUN
    // the same in double, the plain way: y = X W^T + b, BatchNorm over the rows, the activation, and autograd's formulas
    std::vector<double> y((size_t)M * C), wH((size_t)M * C), wdW((size_t)C * Cin, 0.0), wdb(C, 0.0), wdg(C, 0.0), wdbt(C, 0.0), wmean(C, 0.0), wis(C, 0.0), wrm(C), wrv(C);
    for (int i = 0; i < M; ++i)
        for (int c = 0; c < C; ++c) {
            double s = bias.p[c];
            for (int a = 0; a < Cin; ++a) s += (double)X.p[(size_t)i * Cin + a] * W.p[(size_t)c * Cin + a];
            y[(size_t)i * C + c] = s;
        }
    // dW in training is the difference scale (S2 - S1 invstd Sigma w) of two terms that cancel as M -> 2 (two rows normalise to +-1
    // whatever W is): its distance is taken relative to the larger of max |dW| and max |scale S2|, the size of what fp32 subtracts
    std::vector<double> xbar(Cin, 0.0);
    for (int i = 0; i < M; ++i) for (int a = 0; a < Cin; ++a) xbar[a] += (double)X.p[(size_t)i * Cin + a] / M;
    double term = 0.0;
    for (int c = 0; c < C; ++c) {
        double m = 0.0, v = 0.0, is = 0.0, sc = 1.0, sh = 0.0;
        if (mode == TK_MODE_BATCH) {
            for (int i = 0; i < M; ++i) m += y[(size_t)i * C + c] / M;
            for (int i = 0; i < M; ++i) { const double d = y[(size_t)i * C + c] - m; v += d * d / M; }
            wrm[c] = (1.0 - mom) * rm0[c] + mom * m; wrv[c] = (1.0 - mom) * rv0[c] + mom * v * M / (M - 1.0);
        } else if (mode == TK_MODE_RUNNING) { m = rm0[c]; v = rv0[c]; wrm[c] = rm0[c]; wrv[c] = rv0[c]; }
        if (mode != TK_MODE_PLAIN) { is = 1.0 / sqrt(v + eps); sc = gamma.p[c] * is; sh = beta.p[c] - m * sc; }
        wmean[c] = m; wis[c] = is;
        double S0 = 0.0, S1 = 0.0;
        std::vector<double> dz(M);
        for (int i = 0; i < M; ++i) {
            const double z = y[(size_t)i * C + c] * sc + sh;
            wH[(size_t)i * C + c] = act_d(z, act);
            dz[i] = dH.p[(size_t)i * C + c] * dact_d(z, act);
            S0 += dz[i]; S1 += dz[i] * (y[(size_t)i * C + c] - m) * is;
        }
        wdg[c] = S1; wdbt[c] = S0;
        for (int i = 0; i < M; ++i) {
            const double dy = mode == TK_MODE_BATCH ? sc * (dz[i] - S0 / M - (y[(size_t)i * C + c] - m) * is * S1 / M) : sc * dz[i];
            for (int a = 0; a < Cin; ++a) wdW[(size_t)c * Cin + a] += dy * X.p[(size_t)i * Cin + a];
            wdb[c] += dy;
        }
        for (int a = 0; a < Cin && mode == TK_MODE_BATCH; ++a) {
            double s2 = 0.0;
            for (int i = 0; i < M; ++i) s2 += dz[i] * (X.p[(size_t)i * Cin + a] - xbar[a]);
            term = fmax(term, fabs(sc * s2));
        }
    }
    const double eh = worst(H.p, wH), ew = worst(dW.p, wdW, term);
    double e = fmax(eh, ew), eb = 0.0, eg = 0.0, et = 0.0, em = 0.0, ei = 0.0, er = 0.0;
    if (mode == TK_MODE_BATCH) for (int c = 0; c < C; ++c) EXPECT(db.p[c] == 0.f);
    else eb = worst(db.p, wdb);
    if (mode != TK_MODE_PLAIN) {
        eg = worst(dgamma.p, wdg); et = worst(dbeta.p, wdbt); em = worst(bn_save.p + 2 * C, wmean); ei = worst(bn_save.p + 3 * C, wis);
        er = fmax(worst(rm.p, wrm), worst(rv.p, wrv));
    }
    e = fmax(fmax(fmax(e, eb), fmax(eg, et)), fmax(fmax(em, ei), er));
    printf("thin_in (%d, %d, %d) mode %d act %d off %g: np %d/%d/%d ct %d nrl %d; H %.2e  dW %.2e  db %.2e  dgamma %.2e  dbeta %.2e  mean %.2e  invstd %.2e  running %.2e\n",
           M, Cin, C, mode, act, off, g.m_np, g.a_np, g.b_np, g.ct, g.nrl, eh, ew, eb, eg, et, em, ei, er);
    worst_all = fmax(worst_all, e);
    EXPECT(e < 1e-5);
}

static void pool_case(int B, int L, int d, bool nans) {
    TpGeo g;
    EXPECT(tp_geo(B, L, d, g));
    Buf<float> y((size_t)B * L * d), out((size_t)B * 2 * d), dOut((size_t)B * 2 * d), dy((size_t)B * L * d), sh_v(RT_THREADS * 4);
    Buf<int> arg((size_t)B * d), sh_a(RT_THREADS * 4);
    fill(y, 1.f); fill(dOut, 1.f);
    if (L > 3) for (int c = 0; c < d; c += 3) y.p[(size_t)3 * d + c] = y.p[(size_t)2 * d + c] = 2.f;        // a tie at the top: row 2 wins
    if (nans) {
        y.p[(size_t)1 * d + 0] = NAN;                                       // a NaN in row 1 of column 0
        for (int l = 0; l < L; ++l) y.p[(size_t)l * d + 1] = NAN;           // column 1: all NaN
    }
    for (int i = 0; i < (int)dy.n; ++i) dy.p[i] = 7.f;
    // token_pool_fwd_kernel, token_pool_bwd_kernel
    for (int bid = 0; bid < B * g.nqb; ++bid) {
        const int b = bid / g.nqb, cq0 = (bid - b * g.nqb) * g.ct;
        for (int tid = 0; tid < RT_THREADS; ++tid) tp_fwd_1(g, b, cq0, tid, y.p, sh_v.p, sh_a.p);
        for (int tid = 0; tid < RT_THREADS; ++tid) tp_fwd_2(g, b, cq0, tid, y.p, sh_v.p, sh_a.p, out.p, arg.p);
    }
    const long long rows = (long long)B * L;
    const int rb = row_tiles(rows, g.c4).rb, grid = 3;
    for (int bid = 0; bid < grid; ++bid)
        for (long long r0 = (long long)bid * rb; r0 < rows; r0 += (long long)grid * rb) {
            const int n = (int)((rows - r0 < rb ? rows - r0 : (long long)rb) * g.c4);
            for (int tid = 0; tid < RT_THREADS; ++tid)
                for (int it = tid; it < n; it += RT_THREADS) tp_bwd_item(g, r0 + it / g.c4, it % g.c4, dOut.p, arg.p, dy.p);
        }
    for (int b = 0; b < B; ++b)
        for (int c = 0; c < d; ++c) {
            int want = 0;
            for (int l = 1; l < L; ++l) {
                const float v = y.p[((size_t)b * L + l) * d + c];
                if (v == v && (want == 0 || v > y.p[((size_t)b * L + want) * d + c])) want = l;
            }
            if (want == 0) want = 1;                                        // all NaN
            const int a = arg.p[(size_t)b * d + c];
            EXPECT(a == want && a >= 1 && a < L);
            const float m = out.p[(size_t)b * 2 * d + d + c], w = y.p[((size_t)b * L + want) * d + c];
            EXPECT(m == w || (m != m && w != w));
            const float c0 = out.p[(size_t)b * 2 * d + c], y0 = y.p[(size_t)b * L * d + c];
            EXPECT(c0 == y0 || (c0 != c0 && y0 != y0));
            for (int l = 0; l < L; ++l) {
                const float wd = l == 0 ? dOut.p[(size_t)b * 2 * d + c] : l == want ? dOut.p[(size_t)b * 2 * d + d + c] : 0.f;
                EXPECT(dy.p[((size_t)b * L + l) * d + c] == wd);
            }
        }
    printf("token_pool (%d, %d, %d)%s: ct %d nrl %d nqb %d; exact\n", B, L, d, nans ? " with NaNs" : "", g.ct, g.nrl, g.nqb);
}

int main() {
    thin_case(2, 3, 4, TK_MODE_BATCH, TK_ACT_RELU, 0.f);
    thin_case(33, 3, 128, TK_MODE_BATCH, TK_ACT_RELU, 0.f);
    thin_case(257, 6, 36, TK_MODE_BATCH, TK_ACT_RELU, 0.f);
    thin_case(130, 8, 128, TK_MODE_BATCH, TK_ACT_RELU, 0.f);
    thin_case(130, 8, 128, TK_MODE_PLAIN, TK_ACT_GELU, 0.f);
    thin_case(33, 3, 128, TK_MODE_RUNNING, TK_ACT_RELU, 0.f);
    thin_case(257, 6, 36, TK_MODE_BATCH, TK_ACT_NONE, 50.f);                // off-centre input
    pool_case(1, 2, 4, false);
    pool_case(3, 6, 24, false);
    pool_case(2, 65, 384, false);
    pool_case(3, 6, 24, true);
    TkGeo g;
    EXPECT(!tk_geo(8, 9, 8, 9, 0, 0, 0.f, 0.f, g) && !tk_geo(8, 3, 6, 3, 0, 0, 0.f, 0.f, g) && !tk_geo(8, 3, 8, 2, 0, 0, 0.f, 0.f, g) && !tk_geo(8, 3, 8, 3, 2, 0, 0.f, 0.f, g));
    EXPECT(tk_geo(65536, 3, 128, 3, 1, 1, 0.f, 0.f, g) && g.a_np == 1024 && g.m_np == 256 && g.b_np == 512);
    EXPECT(tk_geo(2048, 3, 128, 3, 3, 0, 0.f, 0.f, g) && g.a_np == 256);
    TpGeo t;
    EXPECT(!tp_geo(1, 1, 4, t) && !tp_geo(1, 2, 6, t) && tp_geo(32, 65, 384, t));
    printf("token_host_check: %s, worst relative distance %.2e (thin (2,3,4) (33,3,128) (257,6,36) (130,8,128); pool (1,2,4) (3,6,24) (2,65,384))\n",
           fails ? "FAILED" : "ok", worst_all);
    return fails != 0;
}
