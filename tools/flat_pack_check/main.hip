// Host sanitizer check of the flat optimizer steps' argument checking and table packing (csrc/flat_segs.h: flat_args_ok, flat_pack,
// adam_groups_fill, sgd_groups_fill -- the host code of flat_launch and its entry points in csrc/optim.hip, minus the launches).  A
// stand-alone program that needs no GPU:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/flat_pack_check/main.hip -o build/flat_pack_check && build/flat_pack_check
//
// The tables are heap arrays of exactly nseg / ngroups entries, so a read past either end is an AddressSanitizer report.
#include "../../mlsp_amd/csrc/flat_segs.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int fails = 0;
#define EXPECT(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static void one(int nseg, int ngroups) {
    std::vector<uint32_t> off(nseg), numel(nseg);
    std::vector<const float*> grads(nseg);
    std::vector<uint8_t> tag(nseg);
    uint32_t at = 0;
    long want_tiles = 0;
    for (int i = 0; i < nseg; ++i) {
        off[i] = at;
        numel[i] = 1 + (uint32_t)((i * 2654435761u) % 5000);          // 1 .. 5000 elements: one to three tiles
        at += (numel[i] + 63) / 64 * 64;
        grads[i] = (const float*)(uintptr_t)(4096 + 16 * (size_t)at);
        tag[i] = (uint8_t)(i % ngroups);
        want_tiles += (numel[i] + FLAT_TILE - 1) / FLAT_TILE;
    }
    for (int tagged = 0; tagged < 2; ++tagged) {
        const uint8_t* sg = tagged ? tag.data() : nullptr;
        EXPECT(flat_args_ok(off.data(), numel.data(), grads.data(), sg, nseg, ngroups));
        long tiles = 0;
        int chunks = 0;
        for (int s0 = 0; s0 < nseg; s0 += FLAT_MAX_SEGS, ++chunks) {
            FlatSegs* a = new FlatSegs;                                 // (on the heap: its ends are guarded too)
            const int t = flat_pack(*a, off.data(), numel.data(), grads.data(), sg, nseg, s0);
            EXPECT(a->n == (nseg - s0 < FLAT_MAX_SEGS ? nseg - s0 : FLAT_MAX_SEGS) && a->tile_begin[0] == 0 && a->tile_begin[a->n] == t);
            for (int i = 0; i < a->n; ++i) {
                EXPECT(a->off[i] == off[s0 + i] && a->numel[i] == numel[s0 + i] && a->grad[i] == grads[s0 + i]);
                EXPECT(a->group[i] == (tagged ? tag[s0 + i] : 0));
                EXPECT(a->tile_begin[i + 1] - a->tile_begin[i] == (int)((numel[s0 + i] + FLAT_TILE - 1) / FLAT_TILE));
            }
            tiles += t;
            delete a;
        }
        EXPECT(tiles == want_tiles && chunks == (nseg + FLAT_MAX_SEGS - 1) / FLAT_MAX_SEGS);
    }
    // what is refused: a tag outside the groups (first, last segment), an empty segment, a missing gradient
    for (int where : {0, nseg - 1}) {
        const uint8_t keep = tag[where];
        tag[where] = (uint8_t)ngroups;
        EXPECT(!flat_args_ok(off.data(), numel.data(), grads.data(), tag.data(), nseg, ngroups));
        tag[where] = keep;
        const uint32_t n0 = numel[where];
        numel[where] = 0;
        EXPECT(!flat_args_ok(off.data(), numel.data(), grads.data(), tag.data(), nseg, ngroups));
        numel[where] = n0;
        const float* g0 = grads[where];
        grads[where] = nullptr;
        EXPECT(!flat_args_ok(off.data(), numel.data(), grads.data(), tag.data(), nseg, ngroups));
        grads[where] = g0;
    }
    EXPECT(!flat_args_ok(off.data(), numel.data(), grads.data(), tag.data(), nseg, 0));
    EXPECT(!flat_args_ok(off.data(), numel.data(), grads.data(), tag.data(), nseg, FLAT_MAX_GROUPS + 1));
    EXPECT(!flat_args_ok(off.data(), numel.data(), grads.data(), tag.data(), 0, ngroups));

    std::vector<mlsp_adam_group_t> ag(ngroups);
    std::vector<mlsp_sgd_group_t> sg(ngroups);
    for (int g = 0; g < ngroups; ++g) {
        ag[g] = mlsp_adam_group_t{1e-3 * (g + 1), 0.9, 0.999, g % 2 ? 1e-2 : 0.0, 1e-8, (int64_t)g + 1, g % 2, (float*)(uintptr_t)(256 * (g + 1))};
        sg[g] = mlsp_sgd_group_t{1e-2 * (g + 1), g % 2 ? 0.9 : 0.0, 0.0, 5e-5, g % 2, 0, g % 3 == 0};
    }
    AdamGroups* at_ = new AdamGroups;
    EXPECT(adam_groups_fill(*at_, ag.data(), ngroups) && at_->n == ngroups);
    for (int g = 0; g < ngroups; ++g)
        EXPECT(at_->g[g].lr == ag[g].lr && at_->g[g].step == (float)(g + 1) && at_->g[g].decoupled == g % 2 && at_->g[g].step_out == ag[g].step_out &&
               at_->g[g].bc1 > 0.f && at_->g[g].bc1 <= 1.f && at_->g[g].bc2s > 0.f && at_->g[g].bc2s <= 1.f);
    ag[ngroups - 1].step = 0;
    EXPECT(!adam_groups_fill(*at_, ag.data(), ngroups));
    EXPECT(!adam_groups_fill(*at_, ag.data(), 0) && !adam_groups_fill(*at_, ag.data(), FLAT_MAX_GROUPS + 1) && !adam_groups_fill(*at_, nullptr, 1));
    delete at_;
    SgdGroups* st = new SgdGroups;
    EXPECT(sgd_groups_fill(*st, sg.data(), ngroups, true) && st->n == ngroups);
    for (int g = 0; g < ngroups; ++g)
        EXPECT(st->g[g].mom_on == g % 2 && st->g[g].nesterov == g % 2 && st->g[g].first == (g % 3 == 0) && st->g[g].wd_on == 1 &&
               st->g[g].neg_lr == (float)(-sg[g].lr));
    EXPECT(sgd_groups_fill(*st, sg.data(), ngroups, false) == (ngroups < 2));      // momentum in group 1 and no buffer
    EXPECT(!sgd_groups_fill(*st, sg.data(), 0, true) && !sgd_groups_fill(*st, sg.data(), FLAT_MAX_GROUPS + 1, true));
    delete st;
}

int main() {
    for (int nseg : {1, 96, 97, 200})
        for (int ngroups : {1, 8}) one(nseg, ngroups);
    printf("flat_pack_check: %s (segments 1 / 96 / 97 / 200 x groups 1 / 8)\n", fails ? "FAILED" : "ok");
    return fails != 0;
}
