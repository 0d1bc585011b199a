// Host sanitizer check of the kernels of csrc/gnedge.hip: their bodies (csrc/gnedge_body.h, one function per phase between two barriers)
// run on the host, one call per work-item and phase in the order gnedge.hip runs them, against heap buffers of exactly the sizes the
// Python layer allocates (functional._GnEdgeMax) and "LDS" / workspace heap blocks of exactly the bytes the launches use -- an index past
// either end of anything is an AddressSanitizer report.  The results are also compared with a plain double-precision loop over the edges.
// A stand-alone program that needs no GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/gn_edge_host_check/main.hip -o build/gn_edge_host_check && build/gn_edge_host_check
#include <hip/hip_runtime.h>
#include "../../mlsp_amd/csrc/gnedge_body.h"
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
static void fill(Buf<float>& b, float amp) { for (size_t i = 0; i < b.n; ++i) b.p[i] = rnd() * amp; }
static double worst(const float* got, const std::vector<double>& want) {
    double e = 0.0, m = 1e-30;
    for (size_t i = 0; i < want.size(); ++i) { e = fmax(e, fabs((double)got[i] - want[i])); m = fmax(m, fabs(want[i])); }
    return e / m;
}
#define ALL_THREADS(call) for (int tid = 0; tid < RT_THREADS; ++tid) { call; }

// the walk of RT_FOR_ITEMS (rowtile.h) with a grid of `grid` workgroups
template <typename F>
static void for_items(long long rows, int c4, int grid, F f) {
    const int rb = row_tiles(rows, c4).rb;
    for (int bid = 0; bid < grid; ++bid)
        for (long long r0 = (long long)bid * rb; r0 < rows; r0 += (long long)grid * rb) {
            const int n = (int)((rows - r0 < rb ? rows - r0 : (long long)rb) * c4);
            for (int tid = 0; tid < RT_THREADS; ++tid)
                for (int it = tid; it < n; it += RT_THREADS) f(r0 + it / c4, it % c4);
        }
}

static void edge_case(int B, int Nk, int Nq, int k, int C, int groups, bool hubs) {
    const float eps = 1e-5f, slope = 0.2f;
    GeGeo g;
    EXPECT(ge_geo(B, Nk, Nq, k, C, groups, C, C, eps, slope, g));
    const size_t Pk = (size_t)B * Nk, Pq = (size_t)B * Nq, E = Pq * k;
    Buf<float> u(Pk * C), w(Pq * C), gamma(C), beta(C), out(Pq * C), stats((size_t)B * groups * 2), dOut(Pq * C), du(Pk * C), dw(Pq * C), dgamma(C), dbeta(C);
    Buf<int> idx(E), rev_off(Pk + 1), rev_ent(E);
    Buf<uint8_t> argk(Pq * C);
    fill(u, 2.f); fill(w, 1.f); fill(gamma, 1.f); fill(beta, 0.5f); fill(dOut, 1.f);
    gamma.p[1] = 0.f;
    for (size_t e = 0; e < E; ++e) idx.p[e] = (int)(rnd_u() % (uint32_t)Nk);
    if (hubs)                                              // source 1: named by no edge; source 2: named by every query (slot 0)
        for (size_t e = 0; e < E; ++e) idx.p[e] = e % k == 0 ? 2 : idx.p[e] == 1 ? 3 : idx.p[e];
    g.u = u.p; g.w = w.p; g.idx = idx.p; g.gamma = gamma.p; g.beta = beta.p;
    // the reverse index in mlsp_group_reverse's format: per source row, (i local << 8) | s ascending
    {
        size_t at = 0;
        for (size_t j = 0; j < Pk; ++j) {
            rev_off.p[j] = (int)at;
            const size_t b = j / Nk;
            for (int il = 0; il < Nq; ++il)
                for (int s = 0; s < k; ++s)
                    if (idx.p[(b * Nq + il) * k + s] == (int)(j % Nk)) rev_ent.p[at++] = (il << 8) | s;
        }
        rev_off.p[Pk] = (int)at;
        EXPECT(at == E);
    }
    // forward: gn_edge_stats_kernel, gn_edge_stats_finalize_kernel, gn_edge_apply_kernel
    {
        Buf<double> part(ge_fwd_ws_doubles(g)), sh(RT_THREADS * 2);
        for (int bid = 0; bid < B * g.np; ++bid) {
            const int b = bid / g.np, p = bid - b * g.np;
            for (int cq0 = 0; cq0 < g.c4; cq0 += g.ct) {
                ALL_THREADS(ge_stats_1(g, b, p, cq0, tid, sh.p));
                ALL_THREADS(ge_stats_2(g, b, p, cq0, tid, sh.p, part.p));
            }
        }
        for (long long t = 0; t < (long long)(B * groups + RT_THREADS - 1) / RT_THREADS * RT_THREADS; ++t) ge_stats_fin(g, t, part.p, stats.p);
        for_items((long long)Pq, g.c4, 3, [&](long long i, int cq) { ge_apply_item(g, i, cq, stats.p, out.p, argk.p); });
    }
    // backward: gn_edge_bsum_kernel, gn_edge_bfin_cloud_kernel, gn_edge_bfin_param_kernel, gn_edge_bwd_dw_kernel, gn_edge_bwd_du_kernel
    {
        Buf<float> chpart(ge_bwd_ws_floats(g)), sh(RT_THREADS * 8), ab((size_t)B * groups * 2);
        Buf<double> cloud(ge_bwd_ws_doubles(g));
        for (int bid = 0; bid < B * g.np; ++bid) {
            const int b = bid / g.np, p = bid - b * g.np;
            for (int cq0 = 0; cq0 < g.c4; cq0 += g.ct) {
                ALL_THREADS(ge_bsum_1(g, b, p, cq0, tid, stats.p, dOut.p, argk.p, sh.p));
                ALL_THREADS(ge_bsum_2(g, b, p, cq0, tid, sh.p, chpart.p));
            }
        }
        for (int b = 0; b < B; ++b) {
            ALL_THREADS(ge_bfin_1(g, b, tid, chpart.p, cloud.p));
            ALL_THREADS(ge_bfin_2(g, b, tid, cloud.p, ab.p));
        }
        for (int c = 0; c < (C + RT_THREADS - 1) / RT_THREADS * RT_THREADS; ++c) ge_bfin_param(g, c, cloud.p, dgamma.p, dbeta.p);
        for_items((long long)Pq, g.c4, 2, [&](long long i, int cq) { ge_bwd_dw_item(g, i, cq, stats.p, ab.p, dOut.p, argk.p, dw.p); });
        for_items((long long)Pk, g.c4, 2, [&](long long j, int cq) { ge_bwd_du_item(g, j, cq, stats.p, ab.p, dOut.p, argk.p, rev_off.p, rev_ent.p, du.p); });
    }
    // the same in double over the edges, the plain way (the slot is the kernel's; that it attains the optimum is checked)
    const int Cg = C / groups;
    const double n = (double)Cg * Nq * k;
    std::vector<double> wout(Pq * C), wdu(Pk * C, 0.0), wdw(Pq * C, 0.0), wdg(C, 0.0), wdb(C, 0.0), wstats((size_t)B * groups * 2);
    auto Y = [&](size_t i, int s, int c) { return (double)u.p[((i / Nq) * Nk + idx.p[i * k + s]) * C + c] + (double)w.p[i * C + c]; };
    for (int b = 0; b < B; ++b)
        for (int gr = 0; gr < groups; ++gr) {
            double m = 0.0, v = 0.0;
            for (int il = 0; il < Nq; ++il) for (int s = 0; s < k; ++s) for (int c = gr * Cg; c < (gr + 1) * Cg; ++c) m += Y((size_t)b * Nq + il, s, c) / n;
            for (int il = 0; il < Nq; ++il) for (int s = 0; s < k; ++s) for (int c = gr * Cg; c < (gr + 1) * Cg; ++c) { const double d = Y((size_t)b * Nq + il, s, c) - m; v += d * d / n; }
            const double rs = 1.0 / sqrt(v + eps);
            wstats[((size_t)b * groups + gr) * 2] = m; wstats[((size_t)b * groups + gr) * 2 + 1] = rs;
            double A = 0.0, Bm = 0.0;
            for (int il = 0; il < Nq; ++il)
                for (int c = gr * Cg; c < (gr + 1) * Cg; ++c) {
                    const size_t i = (size_t)b * Nq + il;
                    const int a = argk.p[i * C + c];
                    EXPECT(a < k);
                    double best = -1e300;
                    for (int s = 0; s < k; ++s) { const double z = (Y(i, s, c) - m) * rs * gamma.p[c] + beta.p[c]; best = fmax(best, z > 0 ? z : z * slope); }
                    const double yh = (Y(i, a, c) - m) * rs, z = yh * gamma.p[c] + beta.p[c];
                    wout[i * C + c] = z > 0 ? z : z * slope;
                    EXPECT(fabs(wout[i * C + c] - best) <= 1e-5 * (1.0 + fabs(best)));
                    const double dz = dOut.p[i * C + c] * (z > 0 ? 1.0 : slope);
                    wdg[c] += dz * yh; wdb[c] += dz;
                    A += gamma.p[c] * dz / n; Bm += gamma.p[c] * dz * yh / n;
                }
            for (int il = 0; il < Nq; ++il)
                for (int c = gr * Cg; c < (gr + 1) * Cg; ++c) {
                    const size_t i = (size_t)b * Nq + il;
                    const int a = argk.p[i * C + c];
                    const double za = (Y(i, a, c) - m) * rs * gamma.p[c] + beta.p[c], dz = dOut.p[i * C + c] * (za > 0 ? 1.0 : slope);
                    for (int s = 0; s < k; ++s) {
                        const double dy = rs * ((s == a ? gamma.p[c] * dz : 0.0) - A - (Y(i, s, c) - m) * rs * Bm);
                        wdw[i * C + c] += dy;
                        wdu[((size_t)b * Nk + idx.p[i * k + s]) * C + c] += dy;
                    }
                }
        }
    const double es = worst(stats.p, wstats), eo = worst(out.p, wout), eu = worst(du.p, wdu), ew = worst(dw.p, wdw), eg = worst(dgamma.p, wdg),
                 eb = worst(dbeta.p, wdb);
    printf("gn_edge (%d, %d, %d, %d, %d, %d): np %d, ct %d, rl %d; stats %.2e  out %.2e  du %.2e  dw %.2e  dgamma %.2e  dbeta %.2e\n", B, Nk, Nq, k, C,
           groups, g.np, g.ct, g.rl, es, eo, eu, ew, eg, eb);
    const double e = fmax(fmax(fmax(es, eo), fmax(eu, ew)), fmax(eg, eb));
    worst_all = fmax(worst_all, e);
    EXPECT(e < 1e-5);
    if (hubs)
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < C; ++c) EXPECT(du.p[((size_t)b * Nk + 1) * C + c] == 0.f && rev_off.p[(size_t)b * Nk + 2] == rev_off.p[(size_t)b * Nk + 1]);
}

int main() {
    edge_case(1, 4, 4, 4, 16, 4, false);
    edge_case(2, 5, 67, 3, 48, 4, false);
    edge_case(1, 8, 16, 16, 512, 4, true);
    edge_case(2, 8, 70, 2, 512, 4, false);                  // five row chunks per cloud: the partials and their finalisers
    GeGeo g;
    EXPECT(!ge_geo(1, 8, 8, 4, 24, 4, 24, 24, 1e-5f, 0.2f, g) && !ge_geo(1, 8, 8, 65, 16, 4, 16, 16, 1e-5f, 0.2f, g) && !ge_geo(1, 8, 8, 0, 16, 4, 16, 16, 1e-5f, 0.2f, g) &&
           !ge_geo(1, 8, 8, 4, 16, 4, 18, 16, 1e-5f, 0.2f, g) && !ge_geo(1, 8, 8, 4, 16, 4, 16, 12, 1e-5f, 0.2f, g));
    EXPECT(ge_geo(32, 256, 512, 4, 512, 4, 512, 512, 1e-5f, 0.2f, g) && ge_geo(1, 64, 64, 64, 16, 4, 16, 16, 1e-5f, 0.2f, g) && ge_geo(2, 8, 8, 4, 4096, 4, 4096, 4096, 1e-5f, 0.2f, g));
    printf("gn_edge_host_check: %s, worst relative distance %.2e (shapes (1,4,4,4,16,4) (2,5,67,3,48,4) (1,8,16,16,512,4) (2,8,70,2,512,4))\n", fails ? "FAILED" : "ok", worst_all);
    return fails != 0;
}
