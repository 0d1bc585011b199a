// Host check of the kNN dispatch plan (mlsp_amd/csrc/knn_plan.h): the one function that decides which kernel a search of a given shape
// runs on.  Two parts:
//   sweep   over a grid of shapes x pitches x alignments x plane offers: every plan that is not refused fits the 160 KiB of LDS, takes no
//           more planes than were offered, runs v5 (alone or behind the wide kernel) on whole 128-query chunks only, launches a sane grid;
//           the knn6*_supported predicates equal their statements (the family of the plan with every byte of planes on offer); and a
//           refused plan is the VALU kernel's.  Every label the sweep reaches is printed as a "reach" line.
//   plans   one "plan" line per line of stdin  `B N C k ld x16 planes_avail planes16`  (tests/test_knn_plan_cpu.py pins the family each
//           test shape reaches with them).
// Labels: family[/CT[/flags]] -- VEX | V6/CT | V6W_V5/CT/v5=CT[,vec][,res] | V5/CT[/vec][,res][,kb] | V4/CT[/vec] | V3/CT[/vec] |
// VALU/KMAX[/c3].  A stand-alone program that needs no GPU and no HIP header:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/knn_plan_host_check/main.cpp
//       -o build/knn_plan_host_check && build/knn_plan_host_check < /dev/null
#include "../../mlsp_amd/csrc/knn_plan.h"
#include <set>
#include <stdio.h>
#include <string>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { if (++fails < 25) printf("FAILED line %d: %s  (B=%d N=%d C=%d k=%d ld=%d)\n", __LINE__, #c, q.B, q.N, q.C, q.k, q.ld); } } while (0)

static std::string flags(std::initializer_list<const char*> on) {
    std::string s;
    for (const char* f : on) if (f) { s += s.empty() ? "/" : ","; s += f; }
    return s;
}
// with_vec = false: the label without the load-width flags (what the coverage of the pins is counted in)
static std::string label(const KnnPlan& p, bool with_vec = true) {
    if (p.status != MLSP_OK) return p.status == MLSP_ERR_ARG ? "ERR_ARG" : "ERR_UNSUPPORTED";
    const Knn5Plan& v = p.v5;
    switch (p.family) {
    case KNN_FAM_VEX: return "VEX";
    case KNN_FAM_V6: return "V6/" + std::to_string(p.CT);
    case KNN_FAM_V6W_V5: return "V6W_V5/" + std::to_string(p.CT) + "/v5=" + std::to_string(v.CT) + (with_vec && v.vec ? ",vec" : "") + (v.res ? ",res" : "");
    case KNN_FAM_V5: return "V5/" + std::to_string(p.CT) + flags({with_vec && v.vec ? "vec" : nullptr, v.res ? "res" : nullptr, v.kb ? "kb" : nullptr});
    case KNN_FAM_V4: return "V4/" + std::to_string(p.CT) + flags({with_vec && p.vec ? "vec" : nullptr});
    case KNN_FAM_V3: return "V3/" + std::to_string(p.CT) + flags({with_vec && p.vec ? "vec" : nullptr});
    default: return "VALU/" + std::to_string(p.KMAX) + flags({p.CT == 3 ? "c3" : nullptr});
    }
}

static void sweep() {
    static const int Bs[] = {1, 3, 8, 32};
    static const int Ns[] = {1, 20, 33, 100, 127, 128, 150, 256, 300, 384, 1024, 1152, 2048, 3584, 4096, 4224, 8192};
    static const int Cs[] = {1, 3, 4, 5, 16, 17, 64, 65, 100, 128, 129, 200, 256, 257, 400};
    static const int ks[] = {1, 7, 20, 21, 24, 25, 32, 33, 40, 41, 64, 65};
    std::set<std::string> reach;
    long points = 0, ok = 0;
    for (int B : Bs) for (int N : Ns) for (int C : Cs) for (int k : ks) for (int pitch = 0; pitch < 3; ++pitch) for (int x16 = 0; x16 < 2; ++x16) {
        KnnAsk q;
        q.B = B; q.N = N; q.C = C; q.k = k; q.x16 = x16 != 0;
        q.ld = pitch == 0 ? C : (C + 3) / 4 * 4 + (pitch == 1 ? 4 : 1);
        const int P = B * N;
        const size_t offers[] = {0, knn6_vex_bytes(P) - 1, knn6_vex_bytes(P), knn6_plane_bytes(P, C) - 1, knn6_plane_bytes(P, C), (size_t)-1};
        for (size_t avail : offers) for (int p16 = 0; p16 < 2; ++p16) {
            q.planes_avail = avail; q.planes16 = p16 != 0;
            const KnnPlan p = knn_plan(q);
            ++points;
            if (k > N) EXPECT(p.status == MLSP_ERR_ARG);
            if (p.status != MLSP_OK) {      // refused: an argument, or a shape only the VALU kernel is left for and cannot hold
                EXPECT(p.status == MLSP_ERR_ARG ? k > N : p.status == MLSP_ERR_UNSUPPORTED && p.family == KNN_FAM_VALU && (k > 40 || p.lds > KNN_LDS_MAX));
                continue;
            }
            ++ok;
            reach.insert(label(p, false));
            EXPECT(p.lds > 0 && p.lds <= KNN_LDS_MAX);
            EXPECT(p.plane_bytes <= avail && (p.plane_bytes == 0 || q.planes16));
            EXPECT(p.block == 256 || p.block == 512);
            EXPECT(p.grid_x >= 1 && p.grid_y >= 1 && (size_t)p.grid_x * p.grid_y * (p.block == 512 ? 128 : p.family == KNN_FAM_VALU ? 64 : 128) >= (size_t)P);
            const bool six = p.family == KNN_FAM_VEX || p.family == KNN_FAM_V6 || p.family == KNN_FAM_V6W_V5;
            EXPECT(p.norm_pass == !six && (p.plane_bytes != 0) == six);
            EXPECT(p.v5.ok == (p.family == KNN_FAM_V5 || p.family == KNN_FAM_V6W_V5));
            if (p.v5.ok) EXPECT(N % 128 == 0 && p.v5.lds > 0 && p.v5.lds <= KNN_LDS_MAX && p.v5.grid_x == (unsigned)(N / 128) * B && !(p.v5.CT == 128 && p.v5.kb && !p.v5.vec));
            if (six) EXPECT(N % 128 == 0 && N <= 4096 && k <= (p.family == KNN_FAM_V6W_V5 ? K6W_KMAX : K6_KMAX));
            if (p.family == KNN_FAM_V4) EXPECT(N >= 256 && k <= 32 && C <= 128 && !knn5_plan(q).ok);
            if (p.family == KNN_FAM_V3) EXPECT(k <= 32 && C <= 256 && p.lds == knn3_lds_bytes(p.CT) && p.CT >= C);
            if (p.family == KNN_FAM_VALU) EXPECT(k <= p.KMAX && (p.CT == 3) == (C == 3));
        }
        // the predicates are statements over the plan of the shape with contiguous aligned rows and every byte of planes on offer
        KnnAsk a = knn_q(B, N, C, k);
        const KnnPlan p = knn_plan(a);
        const bool okp = p.status == MLSP_OK;
        EXPECT(knn_q_vex_supported(B, N, C, k) == (okp && p.family == KNN_FAM_VEX));
        EXPECT((knn_q_v6_supported(B, N, C, k) && C > 16) == (okp && p.family == KNN_FAM_V6));                 // (C <= 16: the kernel would take it, the plan keeps v5 / VEX)
        EXPECT((knn_q_v6w_supported(B, N, C, k) && knn5_plan(a).ok) == (okp && p.family == KNN_FAM_V6W_V5));   // (only where v5 can stand behind it)
    }
    for (const std::string& s : reach) printf("reach %s\n", s.c_str());
    printf("sweep: %ld points, %ld plans not refused, %zu labels\n", points, ok, reach.size());
    KnnAsk q;
    EXPECT(points == 4L * 17 * 15 * 12 * 3 * 2 * 6 * 2 && ok > points / 4 && reach.size() >= 30);
}

int main() {
    sweep();
    KnnAsk q;
    int x16, p16;
    unsigned long long avail;
    while (scanf("%d %d %d %d %d %d %llu %d", &q.B, &q.N, &q.C, &q.k, &q.ld, &x16, &avail, &p16) == 8) {
        q.x16 = x16 != 0; q.planes_avail = (size_t)avail; q.planes16 = p16 != 0;
        const KnnPlan p = knn_plan(q);
        printf("plan %d %d %d %d -> %s lds %zu grid %u,%u block %u planes %zu norm %d\n", q.B, q.N, q.C, q.k, label(p).c_str(), p.lds, p.grid_x, p.grid_y, p.block,
               p.plane_bytes, (int)p.norm_pass);
    }
    if (fails) { printf("knn_plan_host_check: %d FAILED\n", fails); return 1; }
    printf("knn_plan_host_check: ok\n");
    return 0;
}
