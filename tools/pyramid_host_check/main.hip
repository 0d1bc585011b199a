// Host sanitizer check of the kernels of csrc/pyramid.hip: their bodies (csrc/pyramid_body.h) run on the host, one call per work-item and
// phase in the order pyramid.hip runs them, against heap buffers of exactly the sizes the Python layer allocates (functional._Interp3Add,
// _CloudMean) and an "LDS" heap block of exactly the bytes the launch uses -- an index past either end of anything is an AddressSanitizer
// report.  The results are also compared with a plain double-precision loop.  A stand-alone program that needs no GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/pyramid_host_check/main.hip -o build/pyramid_host_check && build/pyramid_host_check
#include <hip/hip_runtime.h>
#include "../../mlsp_amd/csrc/pyramid_body.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fails = 0;
static double worst_all = 0.0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// exact-size, 16-byte-aligned heap array (n == 0: no array at all, as the NULL the Python layer passes)
template <typename T>
struct Buf {
    T* p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (n) { if (posix_memalign((void**)&p, 16, n * sizeof(T))) abort(); for (size_t i = 0; i < n; ++i) p[i] = T(0); } }
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
};
static uint32_t rng_state = 2463534242u;
static uint32_t rnd_u() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd() { return (float)(rnd_u() & 0xffff) / 32768.0f - 1.0f; }
static void fill(Buf<float>& b, float amp, float off = 0.f) { for (size_t i = 0; i < b.n; ++i) b.p[i] = off + rnd() * amp; }
// max |got - want| / max |want|
static double worst(const float* got, const std::vector<double>& want) {
    double e = 0.0, m = 1e-30;
    for (size_t i = 0; i < want.size(); ++i) { e = fmax(e, fabs((double)got[i] - want[i])); m = fmax(m, fabs(want[i])); }
    return e / m;
}
// the item loop of pyramid.hip (RT_FOR_ITEMS of rowtile.h) on a grid of `grid` workgroups
template <typename F>
static void item_loop(const PyGeo& g, long long rows, int grid, F f) {
    const int rb = row_tiles(rows, g.c4).rb;
    for (int bid = 0; bid < grid; ++bid)
        for (long long r0 = (long long)bid * rb; r0 < rows; r0 += (long long)grid * rb) {
            const int n = (int)((rows - r0 < rb ? rows - r0 : (long long)rb) * g.c4);
            for (int tid = 0; tid < RT_THREADS; ++tid)
                for (int it = tid; it < n; it += RT_THREADS) f(r0 + it / g.c4, it % g.c4);
        }
}
static void cloud_sum(const PyGeo& g, double div, const float* X, float* out) {
    Buf<double> sh((size_t)RT_THREADS * 4);
    for (int bid = 0; bid < g.B * g.nqb; ++bid) {
        const int b = bid / g.nqb, cq0 = (bid - b * g.nqb) * g.ct;
        for (size_t i = 0; i < sh.n; ++i) sh.p[i] = 1e300;                  // (what another workgroup left behind)
        for (int tid = 0; tid < RT_THREADS; ++tid) py_cloud_sum_1(g, b, cq0, tid, X, sh.p);
        for (int tid = 0; tid < RT_THREADS; ++tid) py_cloud_sum_2(g, b, cq0, tid, sh.p, div, out);
    }
}

static void interp_case(int B, int N, int S, int C) {
    PyGeo g;
    EXPECT(py_geo(B, N, S, C, g));
    const bool one = S == 1;
    Buf<float> feat((size_t)B * S * C), add((size_t)B * N * C), out((size_t)B * N * C), dout((size_t)B * N * C), dfeat((size_t)B * S * C),
        dist(one ? 0 : (size_t)B * N * 3);
    Buf<int> idx(one ? 0 : (size_t)B * N * 3), rev_off(one ? 0 : (size_t)B * S + 1), rev_ent(one ? 0 : (size_t)B * N * 3);
    fill(feat, 1.f); fill(add, 1.f); fill(dout, 1.f);
    for (size_t i = 0; i < out.n; ++i) out.p[i] = 7.f;
    for (size_t i = 0; i < dfeat.n; ++i) dfeat.p[i] = 7.f;
    if (!one) {
        for (size_t pn = 0; pn < (size_t)B * N; ++pn) {
            int a = rnd_u() % S, b = rnd_u() % (S - 1), c = rnd_u() % (S - 2);      // three distinct rows, ascending distances
            if (b >= a) ++b;
            const int lo = a < b ? a : b, hi = a < b ? b : a;
            if (c >= lo) ++c;
            if (c >= hi) ++c;
            idx.p[pn * 3] = a; idx.p[pn * 3 + 1] = b; idx.p[pn * 3 + 2] = c;
            float d = pn % 5 == 0 ? 0.f : fabsf(rnd()) * 0.1f;                      // (a query on top of a source point: distance 0)
            for (int u = 0; u < 3; ++u) { dist.p[pn * 3 + u] = d; d += fabsf(rnd()) * 0.1f; }
        }
        // the reverse index as mlsp_group_reverse leaves it: per source row, entries n << 8 | slot in ascending order
        std::vector<std::vector<int>> lists((size_t)B * S);
        for (int b = 0; b < B; ++b)
            for (int n = 0; n < N; ++n)
                for (int u = 0; u < 3; ++u) lists[(size_t)b * S + idx.p[((size_t)b * N + n) * 3 + u]].push_back(n << 8 | u);
        int o = 0;
        for (size_t s = 0; s < lists.size(); ++s) { rev_off.p[s] = o; for (int e : lists[s]) rev_ent.p[o++] = e; }
        rev_off.p[lists.size()] = o;
        EXPECT(o == B * N * 3);
    }
    // interp3_add_fwd_kernel;  interp3_add_bwd_kernel | cloud_sum_kernel
    item_loop(g, (long long)B * N, 3, [&](long long r, int cq) { py_interp_add_fwd_item(g, r, cq, feat.p, idx.p, dist.p, add.p, out.p); });
    if (one) cloud_sum(g, 1.0, dout.p, dfeat.p);
    else item_loop(g, (long long)B * S, 2, [&](long long r, int cq) { py_interp_add_bwd_item(g, r, cq, dout.p, dist.p, rev_off.p, rev_ent.p, dfeat.p); });
    // the same in double, the plain way
    std::vector<double> wout((size_t)B * N * C), wdf((size_t)B * S * C, 0.0);
    for (int b = 0; b < B; ++b)
        for (int n = 0; n < N; ++n) {
            const size_t pn = (size_t)b * N + n;
            double w[3] = {1.0, 0.0, 0.0}, ws = 1.0;
            int src[3] = {0, 0, 0};
            if (!one) {
                ws = 0.0;
                for (int u = 0; u < 3; ++u) { w[u] = 1.0 / ((double)dist.p[pn * 3 + u] + 1e-8); ws += w[u]; src[u] = idx.p[pn * 3 + u]; }
            }
            for (int c = 0; c < C; ++c) {
                double s = add.p[pn * C + c];
                for (int u = 0; u < (one ? 1 : 3); ++u) {
                    s += w[u] / ws * feat.p[((size_t)b * S + src[u]) * C + c];
                    wdf[((size_t)b * S + src[u]) * C + c] += w[u] / ws * dout.p[pn * C + c];
                }
                wout[pn * C + c] = s;
            }
        }
    const double eo = worst(out.p, wout), ed = worst(dfeat.p, wdf);
    printf("interp3_add (%d, %d, %d, %d): out %.2e  dfeat %.2e\n", B, N, S, C, eo, ed);
    worst_all = fmax(worst_all, fmax(eo, ed));
    EXPECT(eo < 2e-6 && ed < 2e-6);
}

static void mean_case(int B, int N, int C, float off) {
    PyGeo g;
    EXPECT(py_geo(B, N, 1, C, g));
    Buf<float> X((size_t)B * N * C), out((size_t)B * C), dOut((size_t)B * C), dX((size_t)B * N * C);
    fill(X, 1.f, off); fill(dOut, 1.f);
    for (size_t i = 0; i < dX.n; ++i) dX.p[i] = 7.f;
    // cloud_sum_kernel, cloud_mean_bwd_kernel
    cloud_sum(g, (double)N, X.p, out.p);
    item_loop(g, (long long)B * N, 3, [&](long long r, int cq) { py_cloud_mean_bwd_item(g, r, cq, dOut.p, dX.p); });
    std::vector<double> wo((size_t)B * C, 0.0), wd((size_t)B * N * C);
    for (int b = 0; b < B; ++b)
        for (int n = 0; n < N; ++n)
            for (int c = 0; c < C; ++c) {
                wo[(size_t)b * C + c] += (double)X.p[((size_t)b * N + n) * C + c] / N;
                wd[((size_t)b * N + n) * C + c] = (double)dOut.p[(size_t)b * C + c] / N;
            }
    const double eo = worst(out.p, wo), ed = worst(dX.p, wd);
    if (N == 1) for (size_t i = 0; i < out.n; ++i) EXPECT(out.p[i] == X.p[i] && dX.p[i] == dOut.p[i]);
    printf("cloud_mean (%d, %d, %d) off %g: ct %d nrl %d nqb %d; out %.2e  dX %.2e\n", B, N, C, off, g.ct, g.nrl, g.nqb, eo, ed);
    worst_all = fmax(worst_all, fmax(eo, ed));
    EXPECT(eo < 1e-7 && ed < 1e-7);
}

int main() {
    interp_case(1, 5, 1, 4);
    interp_case(2, 48, 3, 32);
    interp_case(3, 130, 17, 36);
    interp_case(2, 300, 1, 36);                                             // the S == 1 backward over more rows than row lanes
    interp_case(1, 40, 9, 4096);                                            // one row per tile
    mean_case(1, 1, 4, 0.f);
    mean_case(3, 130, 36, 0.f);
    mean_case(2, 1024, 512, 0.f);
    mean_case(2, 300, 68, 50.f);                                            // off-centre rows, a partial last quad block
    PyGeo g;
    EXPECT(!py_geo(1, 5, 1, 6, g) && !py_geo(1, 5, 1, 2, g) && !py_geo(0, 5, 1, 4, g) && !py_geo(1, 0, 1, 4, g) && !py_geo(1, 5, 0, 4, g));
    EXPECT(py_geo(2, 1024, 1, 512, g) && g.ct == 16 && g.nrl == 16 && g.nqb == 8);
    EXPECT(py_geo(3, 130, 17, 36, g) && g.ct == 9 && g.nrl == 28 && g.nqb == 1);
    printf("pyramid_host_check: %s, worst relative distance %.2e (interp3_add (1,5,1,4) (2,48,3,32) (3,130,17,36) (2,300,1,36) (1,40,9,4096); "
           "cloud_mean (1,1,4) (3,130,36) (2,1024,512) (2,300,68))\n", fails ? "FAILED" : "ok", worst_all);
    return fails != 0;
}
