// Host sanitizer check of batchprep_kernel (csrc/batchprep.hip): its phases (csrc/batchprep_body.h) run on the host, one call per thread
// and phase in the order the kernel runs them, against heap buffers of exactly the sizes the Python layer allocates (mlsp_amd/data.py: raw
// [B][Nmax][ld], start [B], Rpre / Rpost [B][9], noise [B][S][3], out [B][S][3], idx [B][S]) and an "LDS" heap block of exactly the bytes
// the launch asks for -- an index past either end of anything is an AddressSanitizer report.  The DPP arg-max of the sampling loop is a
// plain maximum over the same keys here.  The results are compared with a plain double-precision loop.  Stand-alone, needs no GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/batchprep_host_check/main.hip -o build/batchprep_host_check && build/batchprep_host_check
#include <hip/hip_runtime.h>
#include "../../mlsp_amd/csrc/batchprep_body.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

static int fails = 0;
static double worst_unit = 0.0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

template <typename T>
struct Buf {
    T* p; size_t n;
    explicit Buf(size_t n_) : p(nullptr), n(n_) { if (n) { if (posix_memalign((void**)&p, 16, n * sizeof(T))) abort(); memset(p, 0, n * sizeof(T)); } }
    ~Buf() { free(p); }
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
};
static uint32_t rng_state = 2463534242u;
static uint32_t rnd_u() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }
static float rnd() { return (float)(rnd_u() & 0xffff) / 32768.0f - 1.0f; }

// the kernel, thread by thread: T threads, cloud b of the launch whose clouds have at most ncap points
static void walk_cloud(int T, int ncap, const float* raw, int ld, int Nmax, int b, int n, int fl, int S, const int* start, const double* Rpre,
                       const double* Rpost, const double* noise, double sigma, double clip, float* out, int* idx) {
    const int NW = T / 64;
    const BpLds L = bp_lds(ncap, S, NW);
    Buf<unsigned char> sm(L.bytes);
    memset(sm.p, 0xa5, L.bytes);                                            // (what another workgroup left behind)
    float* cx = (float*)(sm.p + L.cx);
    double* part = (double*)(sm.p + L.part);
    double* partm = (double*)(sm.p + L.partm);
    double* wsum = (double*)(sm.p + L.wsum);
    double* wmax = (double*)(sm.p + L.wmax);
    unsigned long long* slot = (unsigned long long*)(sm.p + L.slot);
    int* sel = (int*)(sm.p + L.sel);
    const float* xb = raw + (size_t)b * Nmax * ld;
    for (int tid = 0; tid < T; ++tid) for (int j = tid; j < n; j += T) bp_stage(xb, ld, j, cx);
    std::vector<double> c((size_t)T * 3, 0.0), r((size_t)T, 1.0);
    if (!(fl & BP_F_RAW)) {
        for (int tid = 0; tid < T; ++tid) if (tid < BP_LANES) bp_sum_lane(cx, n, tid, part);
        for (int tid = 0; tid < T; ++tid) if (tid < BP_GROUPS) bp_sum_group(part, tid, wsum);
        for (int tid = 0; tid < T; ++tid) { bp_centroid(wsum, n, &c[3 * tid]); if (tid < BP_LANES) bp_max_lane(cx, n, tid, &c[3 * tid], partm); }
        for (int tid = 0; tid < T; ++tid) if (tid < BP_GROUPS) bp_max_group(partm, tid, wmax);
        for (int tid = 0; tid < T; ++tid) r[tid] = bp_radius(wmax);
    }
    const double* R = (fl & BP_F_PRE) ? Rpre + (size_t)b * 9 : nullptr;
    for (int tid = 0; tid < T; ++tid) for (int j = tid; j < n; j += T) bp_norm_rotate(cx, j, fl, &c[3 * tid], r[tid], R);
    std::vector<float> px((size_t)T * BP_PPT, 0.f), py(px), pz(px), dmin((size_t)T * BP_PPT, 0.f);
    for (int tid = 0; tid < T; ++tid)
        for (int u = 0; u < BP_PPT; ++u) {
            const int j = tid + T * u;
            dmin[tid * BP_PPT + u] = j < n ? 1e10f : 0.f;
            if (j < n) { px[tid * BP_PPT + u] = cx[3 * j]; py[tid * BP_PPT + u] = cx[3 * j + 1]; pz[tid * BP_PPT + u] = cx[3 * j + 2]; }
        }
    const bool sample = S < n;
    if (sample) {
        int far = bp_clamp_start(start[b], n);
        for (int i = 0; i < S; ++i) {
            sel[i] = far;                                                    // (thread 0)
            const float fx = cx[3 * far], fy = cx[3 * far + 1], fz = cx[3 * far + 2];
            for (int w = 0; w < NW; ++w) {
                unsigned long long wk = 0ull;                                // the wave's maximum (DPP on the device)
                for (int tid = 64 * w; tid < 64 * w + 64; ++tid)
                    for (int u = 0; u < BP_PPT; ++u) {
                        const unsigned long long k = bp_fps_point(px[tid * BP_PPT + u], py[tid * BP_PPT + u], pz[tid * BP_PPT + u],
                                                                  dmin[tid * BP_PPT + u], fx, fy, fz, tid + T * u);
                        wk = k > wk ? k : wk;
                    }
                slot[(i & 1) * NW + w] = wk;
            }
            unsigned long long best = slot[(i & 1) * NW];
            for (int w = 1; w < NW; ++w) best = slot[(i & 1) * NW + w] > best ? slot[(i & 1) * NW + w] : best;
            far = bp_key_index(best);
        }
    }
    const double* Q = (fl & BP_F_POST) ? Rpost + (size_t)b * 9 : nullptr;
    for (int tid = 0; tid < T; ++tid)
        for (int i = tid; i < S; i += T) {
            const int src = sample ? sel[i] : i;
            const size_t o = (size_t)b * S + i;
            float w[3];
            bp_epilogue(cx, src, fl, Q, (fl & BP_F_JITTER) ? noise + o * 3 : nullptr, sigma, clip, w);
            out[o * 3] = w[0]; out[o * 3 + 1] = w[1]; out[o * 3 + 2] = w[2];
            idx[o] = src;
        }
}

// the plain way: double where the kernel is double, one loop per stage
static void plain_cloud(const float* xb, int ld, int n, int fl, int S, int start, const double* R, const double* Q, const double* nz, double sigma,
                        double clip, std::vector<float>& out, std::vector<int>& idx, std::vector<double>& unit64) {
    std::vector<float> v((size_t)n * 3);
    unit64.assign((size_t)n * 3, 0.0);
    double c[3] = {0, 0, 0}, r2 = 0.0;
    for (int j = 0; j < n; ++j) for (int k = 0; k < 3; ++k) c[k] += xb[(size_t)j * ld + k];
    for (int k = 0; k < 3; ++k) c[k] /= n;
    for (int j = 0; j < n; ++j) {
        double d = 0.0;
        for (int k = 0; k < 3; ++k) d += (xb[(size_t)j * ld + k] - c[k]) * (xb[(size_t)j * ld + k] - c[k]);
        r2 = d > r2 ? d : r2;
    }
    for (int j = 0; j < n; ++j) {
        float u[3];
        for (int k = 0; k < 3; ++k) {
            unit64[(size_t)j * 3 + k] = (fl & BP_F_RAW) ? (double)xb[(size_t)j * ld + k] : (xb[(size_t)j * ld + k] - c[k]) / sqrt(r2);
            u[k] = (float)unit64[(size_t)j * 3 + k];
        }
        for (int k = 0; k < 3; ++k)
            v[(size_t)j * 3 + k] = (fl & BP_F_PRE) ? (float)(((double)u[0] * R[k] + (double)u[1] * R[3 + k]) + (double)u[2] * R[6 + k]) : u[k];
    }
    idx.assign(S, 0);
    if (S < n) {
        std::vector<float> dm(n, 1e10f);
        int far = start;
        for (int i = 0; i < S; ++i) {
            idx[i] = far;
            float best = -1.f; int bi = 0;
            for (int j = 0; j < n; ++j) {
                const float dx = v[3 * j] - v[3 * far], dy = v[3 * j + 1] - v[3 * far + 1], dz = v[3 * j + 2] - v[3 * far + 2];
                const float d = (dx * dx + dy * dy) + dz * dz;
                if (d < dm[j]) dm[j] = d;
                if (dm[j] > best) { best = dm[j]; bi = j; }
            }
            far = bi;
        }
    } else for (int i = 0; i < S; ++i) idx[i] = i;
    out.assign((size_t)S * 3, 0.f);
    for (int i = 0; i < S; ++i) {
        const float* p = &v[(size_t)idx[i] * 3];
        for (int k = 0; k < 3; ++k) {
            float w = (fl & BP_F_POST) ? (float)(((double)p[0] * Q[k] + (double)p[1] * Q[3 + k]) + (double)p[2] * Q[6 + k]) : p[k];
            if (fl & BP_F_JITTER) { double t = sigma * nz[(size_t)i * 3 + k]; t = fmin(fmax(t, -clip), clip); w = (float)((double)w + t); }
            out[(size_t)i * 3 + k] = w;
        }
    }
}

static bool bits_equal(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// one batch as the launcher would run it: every cloud in the kernel width its chunk gets
static void batch_case(const char* what, std::vector<int> counts, int S, std::vector<int> flags, int ld, float off, int nan_cloud = -1) {
    const int B = (int)counts.size();
    int Nmax = 0;
    for (int n : counts) Nmax = n > Nmax ? n : Nmax;
    Buf<float> raw((size_t)B * Nmax * ld), out((size_t)B * S * 3);
    Buf<int> start(B), idx((size_t)B * S);
    Buf<double> Rpre((size_t)B * 9), Rpost((size_t)B * 9), noise((size_t)B * S * 3);
    for (size_t i = 0; i < raw.n; ++i) raw.p[i] = off + rnd();
    if (nan_cloud >= 0) for (int j = 0; j < counts[nan_cloud]; ++j) for (int k = 0; k < 3; ++k) raw.p[((size_t)nan_cloud * Nmax + j) * ld + k] = 0.25f * (k + 1);
    for (int b = 0; b < B; ++b) {
        start.p[b] = b % 3 == 1 ? counts[b] - 1 : (int)(rnd_u() % counts[b]);
        const double a = rnd() * 3.0, q = rnd() * 3.0;
        const double rx[9] = {1, 0, 0, 0, cos(a), -sin(a), 0, sin(a), cos(a)}, rz[9] = {cos(q), -sin(q), 0, sin(q), cos(q), 0, 0, 0, 1};
        for (int e = 0; e < 9; ++e) { Rpre.p[b * 9 + e] = rx[e]; Rpost.p[b * 9 + e] = rz[e]; }
    }
    for (size_t i = 0; i < noise.n; ++i) noise.p[i] = rnd() * 3.0;
    for (size_t i = 0; i < out.n; ++i) out.p[i] = 7.f;
    const int ncap = (Nmax + 1) & ~1, T = Nmax > 256 * BP_PPT ? 1024 : 256;
    double wu = 0.0;
    for (int b = 0; b < B; ++b) {
        walk_cloud(T, ncap, raw.p, ld, Nmax, b, counts[b], flags[b], S, start.p, Rpre.p, Rpost.p, noise.p, 0.01, 0.02, out.p, idx.p);
        std::vector<float> want; std::vector<int> widx; std::vector<double> u64;
        plain_cloud(raw.p + (size_t)b * Nmax * ld, ld, counts[b], flags[b], S, start.p[b], Rpre.p + b * 9, Rpost.p + b * 9,
                    noise.p + (size_t)b * S * 3, 0.01, 0.02, want, widx, u64);
        const bool only_unit = flags[b] == 0 && S == counts[b];
        for (int i = 0; i < S; ++i) {
            EXPECT(idx.p[(size_t)b * S + i] >= 0 && idx.p[(size_t)b * S + i] < counts[b]);
            if (b == nan_cloud) {
                EXPECT(idx.p[(size_t)b * S + i] == (i == 0 || S == counts[b] ? (S == counts[b] ? i : start.p[b]) : 0));
                for (int k = 0; k < 3; ++k) EXPECT(out.p[((size_t)b * S + i) * 3 + k] != out.p[((size_t)b * S + i) * 3 + k]);
                continue;
            }
            if (only_unit)                                                   // the unit cube alone: distance from the double result
                for (int k = 0; k < 3; ++k) wu = fmax(wu, fabs((double)out.p[((size_t)b * S + i) * 3 + k] - u64[(size_t)i * 3 + k]));
            // the plain loop sums the centroid in another order: a last-bit difference of the unit cube may move what follows, so
            // exactness is asked where the unit cube is off (BP_F_RAW) and the distance from the plain result elsewhere
            if (flags[b] & BP_F_RAW) {
                EXPECT(idx.p[(size_t)b * S + i] == widx[i]);
                for (int k = 0; k < 3; ++k) EXPECT(bits_equal(out.p[((size_t)b * S + i) * 3 + k], want[(size_t)i * 3 + k]));
            } else if (idx.p[(size_t)b * S + i] == widx[i]) {
                for (int k = 0; k < 3; ++k) EXPECT(fabs((double)out.p[((size_t)b * S + i) * 3 + k] - want[(size_t)i * 3 + k]) <= 0x1p-22);
            }
        }
    }
    if (wu > 0.0) { worst_unit = fmax(worst_unit, wu); EXPECT(wu <= 0x1p-23); }
    printf("%-44s B %d Nmax %4d S %4d ld %d T %4d%s\n", what, B, Nmax, S, ld, T, fails ? "  FAILED" : "");
}

int main() {
    const int RAW = BP_F_RAW, ALL = BP_F_PRE | BP_F_POST | BP_F_JITTER;
    batch_case("count 1", {1}, 1, {0}, 3, 0.f, 0);                           // one point: r = 0, NaN
    batch_case("unit cube, ragged", {24, 33, 257, 2048}, 24, {0, 0, 0, 0}, 3, 0.f);
    batch_case("unit cube, S == count", {24}, 24, {0}, 3, 0.f);
    batch_case("unit cube, S == count, off-centre", {2048}, 2048, {0}, 3, 50.f);
    batch_case("unit cube, S == count 2049", {2049}, 2049, {0}, 4, 0.f);
    batch_case("unit cube, S == count 8192", {8192}, 8192, {0}, 3, 0.f);
    batch_case("sampling alone, ragged", {24, 33, 257, 2048}, 24, {RAW, RAW, RAW, RAW}, 6, 0.f);
    batch_case("sampling alone 2048 -> 1024", {2048, 2048}, 1024, {RAW, RAW}, 3, 0.f);
    batch_case("sampling alone 2049 -> 16", {2049}, 16, {RAW}, 3, 0.f);
    batch_case("sampling alone 8192 -> 16, ragged", {8192, 33, 2049}, 16, {RAW, RAW, RAW}, 3, 0.f);
    batch_case("S == 1", {257, 33}, 1, {RAW | ALL, RAW}, 3, 0.f);
    batch_case("every stage, unit cube off", {33, 257, 24}, 24, {RAW | ALL, RAW | BP_F_PRE, RAW | BP_F_POST | BP_F_JITTER}, 5, 0.f);
    batch_case("every stage", {2048, 257, 33}, 24, {ALL, BP_F_PRE, BP_F_POST | BP_F_JITTER}, 3, 0.f);
    batch_case("every stage 2048 -> 1024", {2048}, 1024, {ALL}, 3, 0.f);
    batch_case("NaN cloud in the middle", {257, 40, 33}, 24, {ALL, ALL, ALL}, 3, 0.f, 1);
    EXPECT(bp_lds(8192, 8192, 16).bytes <= 150 * 1024);
    EXPECT(bp_clamp_start(-5, 10) == 0 && bp_clamp_start(10, 10) == 9 && bp_clamp_start(3, 10) == 3);
    printf("batchprep_host_check: %s, unit cube at most %.2e from the double result\n", fails ? "FAILED" : "ok", worst_unit);
    return fails != 0;
}
