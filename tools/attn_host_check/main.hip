// Host sanitizer check of the kernels of csrc/attn.hip: their bodies (csrc/attn_body.h, one function per phase between two barriers) run
// on the host, one call per work-item and phase in the order attn.hip runs them, against heap buffers of exactly the sizes the Python
// layer allocates and an "LDS" heap block of exactly the bytes the launch asks for -- an index past either end of anything is an
// AddressSanitizer report.  The results are also compared with a plain double-precision loop.  A stand-alone program that needs no GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/attn_host_check/main.hip -o build/attn_host_check && build/attn_host_check
#include <hip/hip_runtime.h>
#include "../../mlsp_amd/csrc/attn_body.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

// exact-size, 16-byte-aligned heap array (std::vector<float> promises only 4)
struct Buf {
    float* p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (posix_memalign((void**)&p, 16, n * sizeof(float))) abort(); for (size_t i = 0; i < n; ++i) p[i] = 0.f; }
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
};
static uint32_t rng_state = 12345u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return (float)((rng_state >> 8) & 0xffff) / 32768.0f - 1.0f; }
static void fill(Buf& b, float amp) { for (size_t i = 0; i < b.n; ++i) b.p[i] = rnd() * amp; }
static double worst(const float* got, const std::vector<double>& want) {
    double e = 0.0, m = 1e-30;
    for (size_t i = 0; i < want.size(); ++i) { e = fmax(e, fabs((double)got[i] - want[i])); m = fmax(m, fabs(want[i])); }
    return e / m;
}
#define ALL_THREADS(call) for (int tid = 0; tid < RT_THREADS; ++tid) { call; }

static void mhsa_case(int B, int L, int d, int H) {
    const int dh = d / H, ld = 3 * d;
    MhsaGeo g;
    EXPECT(mhsa_geo(B, L, H, dh, ld, ld, 1.0f / sqrtf((float)dh), false, g));
    const size_t rows = (size_t)B * L;
    Buf qkv(rows * ld), out(rows * d), lse((size_t)B * H * L), dout(rows * d), dqkv(rows * ld), lds(mhsa_lds_floats(g));
    fill(qkv, 1.5f); fill(dout, 1.0f);
    const int nblocks = B * H * g.nqb;
    for (int bid = 0; bid < nblocks; ++bid) {                       // mhsa_fwd_kernel
        const MhsaWho o = mhsa_who(g, bid);
        ALL_THREADS(mhsa_stage(g, o, tid, qkv.p, g.ld, d + o.h * dh, qkv.p, g.ld, 2 * d + o.h * dh, lds.p));
        for (int r = 0; r < mhsa_steps(g); ++r) {
            ALL_THREADS(mhsa_fwd_a(g, bid, tid, r, qkv.p, lds.p));
            ALL_THREADS(mhsa_fwd_b(g, bid, tid, r, lds.p));
            ALL_THREADS(mhsa_fwd_c(g, bid, tid, r, lds.p));
            ALL_THREADS(mhsa_fwd_d(g, bid, tid, r, lds.p, out.p, lse.p));
        }
    }
    const int fwd_blocks = nblocks;
    const size_t fwd_lds = mhsa_lds_floats(g);
    EXPECT(mhsa_geo(B, L, H, dh, ld, ld, 1.0f / sqrtf((float)dh), true, g) && g.nqb == 1 && mhsa_lds_floats(g) == fwd_lds);
    for (int bid = 0; bid < B * H; ++bid) {                         // mhsa_bwd_kernel: a workgroup per (cloud, head)
        const MhsaWho o = mhsa_who(g, bid);
        ALL_THREADS(mhsa_stage(g, o, tid, qkv.p, g.ld, d + o.h * dh, qkv.p, g.ld, 2 * d + o.h * dh, lds.p));
        for (int r = 0; r < mhsa_steps(g); ++r) {
            ALL_THREADS(mhsa_bwd_row_a(g, bid, tid, r, qkv.p, dout.p, lds.p));
            ALL_THREADS(mhsa_bwd_row_b(g, bid, tid, r, lse.p, lds.p));
            ALL_THREADS(mhsa_bwd_row_d(g, bid, tid, r, lds.p, dqkv.p));
        }
        ALL_THREADS(mhsa_stage(g, o, tid, qkv.p, g.ld, o.h * dh, dout.p, d, o.h * dh, lds.p));
        ALL_THREADS(mhsa_bwd_col_stats(g, bid, tid, lse.p, lds.p));
        for (int r = 0; r < mhsa_steps(g); ++r) {
            ALL_THREADS(mhsa_bwd_col_a(g, bid, tid, r, qkv.p, lds.p));
            ALL_THREADS(mhsa_bwd_col_b(g, bid, tid, r, lds.p));
            ALL_THREADS(mhsa_bwd_col_d(g, bid, tid, r, lds.p, dqkv.p));
        }
    }
    // the same in double, the plain way
    std::vector<double> wout(rows * d), wlse((size_t)B * H * L), wd(rows * ld, 0.0), P((size_t)L * L), dP((size_t)L * L);
    for (int b = 0; b < B; ++b)
        for (int h = 0; h < H; ++h) {
            const float* q = qkv.p + (size_t)b * L * ld + h * dh;
            const float *k = q + d, *v = q + 2 * d;
            for (int i = 0; i < L; ++i) {
                double mx = -1e300, sum = 0.0;
                for (int j = 0; j < L; ++j) {
                    double s = 0.0;
                    for (int c = 0; c < dh; ++c) s += (double)q[(size_t)i * ld + c] * k[(size_t)j * ld + c];
                    P[(size_t)i * L + j] = s * g.scale;
                    mx = fmax(mx, s * g.scale);
                }
                for (int j = 0; j < L; ++j) sum += (P[(size_t)i * L + j] = exp(P[(size_t)i * L + j] - mx));
                wlse[((size_t)b * H + h) * L + i] = mx + log(sum);
                double delta = 0.0;
                for (int c = 0; c < dh; ++c) {
                    double acc = 0.0;
                    for (int j = 0; j < L; ++j) acc += (P[(size_t)i * L + j] / sum) * v[(size_t)j * ld + c];
                    wout[((size_t)b * L + i) * d + h * dh + c] = acc;
                    delta += acc * dout.p[((size_t)b * L + i) * d + h * dh + c];
                }
                for (int j = 0; j < L; ++j) {
                    double dp = 0.0;
                    for (int c = 0; c < dh; ++c) dp += (double)dout.p[((size_t)b * L + i) * d + h * dh + c] * v[(size_t)j * ld + c];
                    P[(size_t)i * L + j] /= sum;
                    dP[(size_t)i * L + j] = P[(size_t)i * L + j] * (dp - delta);
                }
            }
            for (int i = 0; i < L; ++i)
                for (int j = 0; j < L; ++j)
                    for (int c = 0; c < dh; ++c) {
                        const double ds = dP[(size_t)i * L + j], p = P[(size_t)i * L + j];
                        wd[((size_t)b * L + i) * ld + h * dh + c] += g.scale * ds * k[(size_t)j * ld + c];
                        wd[((size_t)b * L + j) * ld + d + h * dh + c] += g.scale * ds * q[(size_t)i * ld + c];
                        wd[((size_t)b * L + j) * ld + 2 * d + h * dh + c] += p * dout.p[((size_t)b * L + i) * d + h * dh + c];
                    }
        }
    const double eo = worst(out.p, wout), el = worst(lse.p, wlse), ed = worst(dqkv.p, wd);
    printf("mhsa (%d, %d, %d, %d): blocks %d, LDS %zu B, kst %d; out %.2e  lse %.2e  dqkv %.2e\n", B, L, d, H, fwd_blocks,
           mhsa_lds_floats(g) * sizeof(float), g.kst, eo, el, ed);
    EXPECT(eo < 1e-5 && el < 1e-5 && ed < 1e-5);
    EXPECT(mhsa_lds_floats(g) * sizeof(float) <= AB_LDS_MAX);
}

static void ln_case(long long rows, int d, int rps, bool with_add, bool with_scale, bool with_gamma) {
    const int d4 = d / 4;
    const size_t n = (size_t)rows * d;
    Buf x(n), a(with_add ? n : 4), s(with_scale ? (size_t)(rows / rps) : 1), gamma(d), beta(d), U(n), Y(n), mean(rows), rstd(rows), red(2 * AB_WAVES * 64);
    fill(x, 2.f); fill(a, 1.f); fill(gamma, 1.f); fill(beta, 1.f);
    for (size_t i = 0; i < s.n; ++i) s.p[i] = (float)(i % 3) * 0.625f;
    const LnGeo g{rows, d4, rps, 1e-5f, x.p, with_add ? a.p : nullptr, with_scale ? s.p : nullptr, with_gamma ? gamma.p : nullptr, with_gamma ? beta.p : nullptr};
    const int grid = 3;                                              // fewer workgroups than row groups: the grid-stride loop runs
    for (int bid = 0; bid < grid; ++bid)                            // layernorm_fwd_kernel
        for (long long row0 = (long long)bid * AB_WAVES; row0 < rows; row0 += (long long)grid * AB_WAVES) {
            ALL_THREADS(ln_fwd_1(g, row0, tid, with_add ? U.p : nullptr, red.p));
            if (!with_gamma) continue;
            ALL_THREADS(ln_fwd_2(g, row0, tid, red.p));
            ALL_THREADS(ln_fwd_3(g, row0, tid, red.p, Y.p, mean.p, rstd.p));
        }
    std::vector<double> wu(n), wy(n);
    for (long long r = 0; r < rows; ++r) {
        double m = 0.0, v = 0.0;
        for (int c = 0; c < d; ++c) {
            wu[r * d + c] = (double)x.p[r * d + c] + (with_add ? (double)(with_scale ? s.p[r / rps] : 1.f) * a.p[r * d + c] : 0.0);
            m += wu[r * d + c] / d;
        }
        for (int c = 0; c < d; ++c) v += (wu[r * d + c] - m) * (wu[r * d + c] - m) / d;
        for (int c = 0; c < d; ++c) wy[r * d + c] = (wu[r * d + c] - m) / sqrt(v + 1e-5) * gamma.p[c] + beta.p[c];
    }
    if (with_add) EXPECT(worst(U.p, wu) < 1e-6);
    if (!with_gamma) return;
    EXPECT(worst(Y.p, wy) < 1e-5);
    // backward: dx, dadd, the partials and their finaliser (layernorm_bwd_kernel, layernorm_bwd_param_kernel, layernorm_bwd_finalize_kernel)
    Buf dy(n), du(n), dx(n), da(n), dg(d), db(d);
    fill(dy, 1.f); fill(du, 1.f);
    const float* usrc = with_add ? U.p : x.p;
    const LnGeo gb{rows, d4, rps, 0.f, usrc, nullptr, with_scale ? s.p : nullptr, gamma.p, nullptr};
    const LnBwd b{dy.p, du.p, mean.p, rstd.p, dx.p, with_add ? da.p : nullptr};
    for (int bid = 0; bid < grid; ++bid)
        for (long long row0 = (long long)bid * AB_WAVES; row0 < rows; row0 += (long long)grid * AB_WAVES) {
            ALL_THREADS(ln_bwd_1(gb, b, row0, tid, red.p));
            ALL_THREADS(ln_bwd_2(gb, b, row0, tid, red.p));
        }
    const int ct = d4 < RT_THREADS ? d4 : RT_THREADS, rl = RT_THREADS / ct, nparts = 5;
    const long long chunk = (rows + nparts - 1) / nparts;
    Buf part((size_t)nparts * d * 2), sh(RT_THREADS * 8);
    for (int bid = 0; bid < nparts; ++bid) {
        const long long e0 = bid * chunk, e1 = e0 + chunk < rows ? e0 + chunk : rows;
        for (int cq0 = 0; cq0 < d4; cq0 += ct) {
            ALL_THREADS(ln_par_1(gb, b, e0, e1, cq0, ct, rl, tid, sh.p));
            ALL_THREADS(ln_par_2(gb, bid, cq0, ct, rl, tid, sh.p, part.p));
        }
    }
    for (int c = 0; c < (d + RT_THREADS - 1) / RT_THREADS * RT_THREADS; ++c) ln_par_fin(part.p, nparts, d, c, dg.p, db.p);
    std::vector<double> wdx(n), wdg(d, 0.0), wdb(d, 0.0);
    for (long long r = 0; r < rows; ++r) {
        double m = 0.0, v = 0.0, m1 = 0.0, m2 = 0.0;
        for (int c = 0; c < d; ++c) m += wu[r * d + c] / d;
        for (int c = 0; c < d; ++c) v += (wu[r * d + c] - m) * (wu[r * d + c] - m) / d;
        const double rs = 1.0 / sqrt(v + 1e-5);
        for (int c = 0; c < d; ++c) {
            const double xh = (wu[r * d + c] - m) * rs, gg = (double)dy.p[r * d + c] * gamma.p[c];
            m1 += gg / d; m2 += gg * xh / d;
            wdg[c] += dy.p[r * d + c] * xh; wdb[c] += dy.p[r * d + c];
        }
        for (int c = 0; c < d; ++c) {
            const double xh = (wu[r * d + c] - m) * rs, gg = (double)dy.p[r * d + c] * gamma.p[c];
            wdx[r * d + c] = rs * (gg - m1 - xh * m2) + du.p[r * d + c];
        }
    }
    EXPECT(worst(dx.p, wdx) < 1e-5 && worst(dg.p, wdg) < 1e-5 && worst(db.p, wdb) < 1e-5);
    if (with_add) {
        for (size_t i = 0; i < n; ++i) wdx[i] *= with_scale ? s.p[(i / d) / rps] : 1.f;
        EXPECT(worst(da.p, wdx) < 1e-5);
    }
}

static void gelu_case(long long rows, int d) {
    const size_t n = (size_t)rows * d;
    Buf x(n), y(n), dy(n), dx(n);
    fill(x, 10.f); fill(dy, 1.f);
    for (long long t = 0; t < (long long)(n / 4); ++t) { gelu_fwd_quad(x.p, t, y.p); gelu_bwd_quad(dy.p, x.p, t, dx.p); }
    std::vector<double> wy(n), wdx(n);
    for (size_t i = 0; i < n; ++i) {
        const double v = x.p[i], cdf = 0.5 * erfc(-v / sqrt(2.0));
        wy[i] = v * cdf;
        wdx[i] = dy.p[i] * (cdf + v * exp(-0.5 * v * v) / sqrt(2.0 * M_PI));
    }
    EXPECT(worst(y.p, wy) < 1e-6 && worst(dx.p, wdx) < 1e-6);
}

int main() {
    const int shapes[3][4] = {{1, 67, 36, 1}, {3, 2, 16, 4}, {1, 256, 64, 1}};
    for (const auto& s : shapes) {
        const int B = s[0], L = s[1], d = s[2], H = s[3];
        mhsa_case(B, L, d, H);
        for (int v = 0; v < 8; ++v) {
            const bool add = v & 1, sc = v & 2, gm = v & 4;
            if ((sc && !add) || (!gm && !add)) continue;
            ln_case((long long)B * L, d, L, add, sc, gm);
        }
        gelu_case((long long)B * L, 4 * d);
    }
    MhsaGeo g;
    EXPECT(!mhsa_geo(1, 257, 1, 64, 192, 192, 1.f, false, g) && !mhsa_geo(1, 513, 1, 4, 12, 12, 1.f, false, g) && !mhsa_geo(1, 8, 1, 132, 396, 396, 1.f, false, g) &&
           !mhsa_geo(1, 8, 1, 6, 18, 18, 1.f, false, g) && !mhsa_geo(1, 8, 2, 8, 44, 48, 1.f, false, g));
    EXPECT(mhsa_geo(4, 512, 3, 32, 288, 288, 1.f, false, g) && mhsa_geo(1, 128, 1, 128, 384, 384, 1.f, false, g) && mhsa_geo(2, 257, 2, 32, 192, 192, 1.f, false, g));
    printf("attn_host_check: %s (shapes (1,67,36,1) (3,2,16,4) (1,256,64,1))\n", fails ? "FAILED" : "ok");
    return fails != 0;
}
