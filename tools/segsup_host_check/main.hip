// Host sanitizer check of the kernels of csrc/segsup.hip: their bodies (csrc/segsup_body.h) run on the host, one call per work-item and
// phase in the order segsup.hip runs them, against heap buffers of exactly the sizes the Python layer allocates (functional._SegCE,
// _seg_metrics_stats), a workspace of exactly ss_ws_bytes and "LDS" heap blocks of exactly the kernels' __shared__ arrays -- an index
// past either end of anything is an AddressSanitizer report.  The results are also compared with a plain double-precision loop.  A
// stand-alone program that needs no GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/segsup_host_check/main.hip -o build/segsup_host_check && build/segsup_host_check
#include <hip/hip_runtime.h>
#include "../../mlsp_amd/csrc/segsup_body.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fails = 0;
static double worst_loss = 0.0, worst_grad = 0.0;
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

struct Lds { Buf<int> cnt; Buf<double> part, lead, slot_loss, slot_valid, iou; Lds(int C) : cnt(ss_ncnt(C)), part(SS_THREADS), lead(SS_LEADERS), slot_loss(SS_THREADS), slot_valid(SS_THREADS), iou(SS_MAXC) {} };

// seg_ce_fwd_kernel<NQ, VEC> / seg_count_kernel on every workgroup of the grid
template <int NQ, bool VEC>
static void fwd_grid(const SsGeo& g, Lds& L, const float* logits, const long long* labels, double* lse, float* loss_pt, long long* pred, double* csum,
                     int* ccnt) {
    const int nc = ss_ncnt(g.C);
    for (int bid = 0; bid < g.B * g.nch; ++bid) {
        const int b = bid / g.nch, k = bid - b * g.nch;
        for (int i = 0; i < nc; ++i) L.cnt.p[i] = -12345;                   // (what another workgroup left behind)
        for (int t = 0; t < SS_THREADS; ++t) if (t < nc) ss_zero(t, L.cnt.p);
        for (int t = 0; t < SS_THREADS; ++t)
            L.part.p[t] = ss_thread_points(g, b, k, t, [&](size_t row) { return ss_fwd_point<NQ, VEC>(g, row, logits, labels, lse, loss_pt, pred, L.cnt.p); });
        for (int t = 0; t < SS_LEADERS; ++t) ss_sum_leader(L.part.p, t, L.lead.p);
        csum[bid] = ss_sum_chunk(L.lead.p);
        for (int t = 0; t < nc; ++t) ccnt[(size_t)bid * nc + t] = L.cnt.p[t];
    }
}
static void count_grid(const SsGeo& g, Lds& L, const long long* labels, const long long* preds, int* ccnt) {
    const int nc = ss_ncnt(g.C);
    for (int bid = 0; bid < g.B * g.nch; ++bid) {
        const int b = bid / g.nch, k = bid - b * g.nch;
        for (int t = 0; t < nc; ++t) ss_zero(t, L.cnt.p);
        for (int t = 0; t < SS_THREADS; ++t) ss_thread_points(g, b, k, t, [&](size_t row) { ss_count_point(g, row, labels, preds, L.cnt.p); return 0.0; });
        for (int t = 0; t < nc; ++t) ccnt[(size_t)bid * nc + t] = L.cnt.p[t];
    }
}
// seg_finalise_kernel, workgroups 0 .. B
static void finalise(const SsGeo& g, Lds& L, const double* csum, const int* ccnt, double* stats, float* mean) {
    const int nc = ss_ncnt(g.C);
    for (int b = 0; b < g.B; ++b) {
        for (int t = 0; t < nc; ++t) L.cnt.p[t] = ss_fin_counter(g, b, t, ccnt);
        ss_fin_cloud(g, b, L.cnt.p, ss_fin_loss(g, b, csum), L.iou.p, stats);
    }
    double loss = 0.0, valid = 0.0;
    for (int b0 = 0; b0 < g.B; b0 += SS_THREADS) {
        const int nb = g.B - b0 < SS_THREADS ? g.B - b0 : SS_THREADS;
        for (int t = 0; t < nb; ++t) { L.slot_loss.p[t] = ss_fin_loss(g, b0 + t, csum); L.slot_valid.p[t] = (double)ss_fin_counter(g, b0 + t, 0, ccnt); }
        ss_fin_batch_add(L.slot_loss.p, L.slot_valid.p, nb, loss, valid);
    }
    ss_fin_batch(g, loss, valid, stats, mean);
}
// seg_ce_bwd_kernel<VEC>: the item loop of RT_FOR_ITEMS on the launch's grid
static void bwd_grid(const SsGeo& g, bool vec, const float* logits, const long long* labels, const double* lse, const float* g_pt, const float* g_mean,
                     const double* stats, float* dlogits) {
    const int c4 = vec ? g.C / 4 : g.C;
    const long long rows = (long long)g.B * g.N;
    const RowTiles t = row_tiles(rows, c4);
    const float gm = g_pt ? 0.f : ss_mean_scale(g, g_mean, stats);
    for (int bid = 0; bid < t.grid; ++bid)
        for (long long r0 = (long long)bid * t.rb; r0 < rows; r0 += (long long)t.grid * t.rb) {
            const int n = (int)((rows - r0 < t.rb ? rows - r0 : (long long)t.rb) * c4);
            for (int tid = 0; tid < RT_THREADS; ++tid)
                for (int it = tid; it < n; it += RT_THREADS) {
                    const int lr = it / c4;
                    if (vec) ss_bwd_quad(g, (size_t)(r0 + lr), it - lr * c4, logits, labels, lse, g_pt, gm, dlogits);
                    else ss_bwd_scalar(g, (size_t)(r0 + lr), it - lr * c4, logits, labels, lse, g_pt, gm, dlogits);
                }
        }
}

// pitch: row pitch of the logits (>= C); shift: added to every logit; ignore: every `ignore`-th label is -100, one is C + 3
static void ce_case(int B, int N, int C, int pitch, float amp, float shift, int ignore, bool none) {
    Buf<float> logits((size_t)B * N * pitch - (pitch - C));                  // (the last row ends at its C-th element)
    Buf<long long> labels((size_t)B * N), pred((size_t)B * N);
    for (size_t i = 0; i < logits.n; ++i) logits.p[i] = shift + amp * rnd();
    for (size_t i = 0; i < labels.n; ++i) labels.p[i] = (long long)(rnd_u() % (unsigned)C);
    if (ignore) { for (size_t i = 1; i < labels.n; i += ignore) labels.p[i] = -100; labels.p[0] = C + 3; }
    SsGeo g;
    EXPECT(ss_geo(B, N, C, pitch, logits.p, g));
    EXPECT(g.nch <= SS_MAXCHUNKS && (long long)g.nch * g.chunk >= N && (long long)(g.nch - 1) * g.chunk < N);
    Buf<double> lse((size_t)B * N), stats((size_t)(B + 1) * SS_STATS);
    Buf<float> loss_pt(none ? (size_t)B * N : 0), mean(1), dlogits((size_t)B * N * C), g_pt(none ? (size_t)B * N : 0), g_mean(none ? 0 : 1);
    Buf<char> ws(ss_ws_bytes(g));
    double* csum = (double*)ws.p;
    int* ccnt = (int*)(ws.p + ss_ws_cnt_offset(g));
    Lds L(C);
    if (C <= 4 * SS_REGQ) { if (g.vec) fwd_grid<SS_REGQ, true>(g, L, logits.p, labels.p, lse.p, loss_pt.p, pred.p, csum, ccnt);
                            else fwd_grid<SS_REGQ, false>(g, L, logits.p, labels.p, lse.p, loss_pt.p, pred.p, csum, ccnt); }
    else { if (g.vec) fwd_grid<0, true>(g, L, logits.p, labels.p, lse.p, loss_pt.p, pred.p, csum, ccnt);
           else fwd_grid<0, false>(g, L, logits.p, labels.p, lse.p, loss_pt.p, pred.p, csum, ccnt); }
    finalise(g, L, csum, ccnt, stats.p, mean.p);
    for (size_t i = 0; i < g_pt.n; ++i) g_pt.p[i] = rnd();
    if (g_mean.n) g_mean.p[0] = 0.75f;
    bwd_grid(g, g.vec && C % 4 == 0, logits.p, labels.p, lse.p, g_pt.p, g_mean.p, stats.p, dlogits.p);

    // the plain loop
    double total = 0.0, nvalid = 0.0, maxlse = 1.0;
    std::vector<double> want_loss((size_t)B * N, 0.0), want_lse((size_t)B * N);
    for (int b = 0; b < B; ++b) {
        std::vector<long long> tp(C, 0), tr(C, 0), pr(C, 0);
        long long correct = 0, valid = 0;
        double csum_b = 0.0;
        for (int n = 0; n < N; ++n) {
            const size_t row = (size_t)b * N + n;
            const float* x = logits.p + row * pitch;
            int arg = 0;
            for (int c = 1; c < C; ++c) if (x[c] > x[arg]) arg = c;
            double s = 0.0;
            for (int c = 0; c < C; ++c) s += exp((double)x[c] - (double)x[arg]);
            const double l = (double)x[arg] + log(s);
            want_lse[row] = l;
            maxlse = fmax(maxlse, fabs(l));
            EXPECT(pred.p[row] == arg);
            EXPECT(fabs(lse.p[row] - l) <= ldexp(fmax(1.0, fabs(l)), -22));
            const long long lab = labels.p[row];
            if (lab < 0 || lab >= C) continue;
            want_loss[row] = l - (double)x[lab];
            csum_b += want_loss[row];
            ++valid; ++tr[lab]; ++pr[arg];
            if (arg == lab) { ++correct; ++tp[lab]; }
        }
        double iou = 0.0; int present = 0;
        for (int c = 0; c < C; ++c) if (tr[c] + pr[c] > 0) { iou += (double)tp[c] / (double)(tr[c] + pr[c] - tp[c]); ++present; }
        const double* o = stats.p + (size_t)b * SS_STATS;
        EXPECT(fabs(o[0] - csum_b) <= (double)valid * ldexp(maxlse, -22));       // (every point within the per-point bound)
        if (valid) { EXPECT(fabs(o[1] - iou / present) <= 1e-14 && o[2] == (double)correct / (double)valid); }
        else EXPECT(o[1] != o[1] && o[2] != o[2]);
        EXPECT(o[3] == (double)valid);
        total += csum_b; nvalid += (double)valid;
    }
    const double* o = stats.p + (size_t)B * SS_STATS;
    EXPECT(o[1] == nvalid);
    if (nvalid > 0) { EXPECT(fabs(o[0] - total / nvalid) <= ldexp(maxlse, -22)); EXPECT(mean.p[0] == (float)o[0]); }
    else EXPECT(o[0] != o[0]);
    for (size_t row = 0; row < (size_t)B * N; ++row) {
        if (none) { const double e = fabs((double)loss_pt.p[row] - want_loss[row]); worst_loss = fmax(worst_loss, e / maxlse); EXPECT(e <= ldexp(maxlse, -22)); }
        const long long lab = labels.p[row];
        const bool ok = lab >= 0 && lab < C;
        const double gr = none ? (double)g_pt.p[row] : 0.75 / nvalid;
        for (int c = 0; c < C; ++c) {
            const double want = ok ? (exp((double)logits.p[row * pitch + c] - want_lse[row]) - (c == lab ? 1.0 : 0.0)) * gr : 0.0;
            const double e = fabs((double)dlogits.p[row * C + c] - want);
            if (!ok) EXPECT(dlogits.p[row * C + c] == 0.f);
            worst_grad = fmax(worst_grad, e / fmax(fabs(gr), 1e-300));
            EXPECT(e <= ldexp(fabs(gr), -22));
        }
    }
}

// the metrics entry: given predictions, one class absent from both, a prediction outside [0, C)
static void metrics_case(int B, int N, int C) {
    Buf<long long> labels((size_t)B * N), preds((size_t)B * N);
    for (size_t i = 0; i < labels.n; ++i) {
        labels.p[i] = (long long)(rnd_u() % (unsigned)(C > 1 ? C - 1 : 1));
        preds.p[i] = (rnd_u() & 1) ? labels.p[i] : (long long)(rnd_u() % (unsigned)(C > 1 ? C - 1 : 1));
    }
    if (N > 2) { preds.p[1] = C + 5; labels.p[2] = -100; }
    SsGeo g;
    EXPECT(ss_geo(B, N, C, C, nullptr, g));
    Buf<char> ws(ss_ws_bytes(g));
    Buf<double> stats((size_t)(B + 1) * SS_STATS);
    Lds L(C);
    int* ccnt = (int*)(ws.p + ss_ws_cnt_offset(g));
    count_grid(g, L, labels.p, preds.p, ccnt);
    finalise(g, L, nullptr, ccnt, stats.p, nullptr);
    for (int b = 0; b < B; ++b) {
        std::vector<long long> tp(C, 0), tr(C, 0), pr(C, 0);
        long long correct = 0, valid = 0;
        for (int n = 0; n < N; ++n) {
            const long long lab = labels.p[(size_t)b * N + n], p = preds.p[(size_t)b * N + n];
            if (lab < 0 || lab >= C) continue;
            ++valid; ++tr[lab];
            if (p >= 0 && p < C) ++pr[p];
            if (p == lab) { ++correct; ++tp[lab]; }
        }
        double iou = 0.0; int present = 0;
        for (int c = 0; c < C; ++c) if (tr[c] + pr[c] > 0) { iou += (double)tp[c] / (double)(tr[c] + pr[c] - tp[c]); ++present; }
        const double* o = stats.p + (size_t)b * SS_STATS;
        EXPECT(fabs(o[1] - iou / present) <= 1e-14 && o[2] == (double)correct / (double)valid && o[3] == (double)valid && o[0] == 0.0);
    }
}

int main() {
    const int Bs[] = {1, 3}, Ns[] = {1, 255, 256, 257, 513}, Cs[] = {1, 2, 8, 10, 13, 64};
    for (int B : Bs) for (int N : Ns) for (int C : Cs) {
        ce_case(B, N, C, C, 3.f, 0.f, 0, false);
        ce_case(B, N, C, C, 3.f, 0.f, 5, true);
        metrics_case(B, N, C);
    }
    ce_case(2, 257, 8, 12, 3.f, 1e4f, 0, true);               // pitched rows, still quads; the max subtraction
    ce_case(2, 257, 8, 9, 80.f, 0.f, 3, false);               // pitched rows off the 16-byte grid: the scalar path; underflowing exps
    ce_case(1, 5, 10, 10, 3.f, 0.f, 1, false);                // every label ignored but label 0 (= C + 3, ignored too): NaN mean
    ce_case(1, SS_THREADS * SS_MAXCHUNKS + 257, 8, 8, 3.f, 0.f, 7, false);   // two points per thread, a partial last chunk
    ce_case(300, 2, 2, 2, 3.f, 0.f, 0, false);                // more clouds than the finaliser's batch row holds at once
    SsGeo g;
    EXPECT(!ss_geo(1, 1, 0, 0, nullptr, g) && !ss_geo(1, 1, 65, 65, nullptr, g) && !ss_geo(0, 1, 8, 8, nullptr, g) && !ss_geo(1, 0, 8, 8, nullptr, g));
    EXPECT(!ss_geo(1 << 16, 1 << 15, 8, 8, nullptr, g) && !ss_geo(1, 1, 8, 7, nullptr, g));
    // the largest cloud of the contract: the chunk arithmetic stays in range, the last chunk's threads stay inside the cloud
    {
        const int N = 2147483647;
        EXPECT(ss_geo(1, N, 8, 8, nullptr, g) && g.nch >= 1 && g.nch <= SS_MAXCHUNKS && g.chunk == SS_THREADS * g.ppt);
        EXPECT((long long)g.nch * g.chunk >= N && (long long)(g.nch - 1) * g.chunk < N);
        for (int k : {0, g.nch - 1}) for (int t : {0, SS_THREADS - 1}) {
            long long visited = 0; size_t first = ~(size_t)0, last = 0;
            ss_thread_points(g, 0, k, t, [&](size_t row) { ++visited; first = row < first ? row : first; last = row > last ? row : last; return 0.0; });
            const long long n0 = (long long)k * g.chunk, n1 = n0 + g.chunk < N ? n0 + g.chunk : (long long)N;
            EXPECT(visited == (n1 - n0 - t + SS_THREADS - 1) / SS_THREADS && first == (size_t)(n0 + t) && last < (size_t)n1 && last + SS_THREADS >= (size_t)n1);
        }
    }
    printf("segsup_host_check: %s, loss at most %.2e max|lse|, gradient at most %.2e |g| from the double loop\n", fails ? "FAILED" : "ok",
           worst_loss, worst_grad);
    return fails ? 1 : 0;
}
