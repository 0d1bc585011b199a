// The segment table of the flat optimizer steps (optim.hip) and the host code that checks and packs it: plain C++, no device code and no
// HIP call, so that tools/flat_pack_check can run exactly this code under the host sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "../../include/mlsp_hip.h"

#define FLAT_MAX_SEGS 96
#define FLAT_MAX_GROUPS 8
#define FLAT_TILE 2048            // elements per workgroup (256 threads x 2 quads)

struct FlatSegs {
    int n;
    int tile_begin[FLAT_MAX_SEGS + 1];      // first tile of every segment; [n] = total
    unsigned off[FLAT_MAX_SEGS];            // first element of the segment in the flat buffers (a multiple of 4 takes the 16-byte path)
    unsigned numel[FLAT_MAX_SEGS];
    const float* grad[FLAT_MAX_SEGS];       // the segment's gradient, contiguous
    unsigned char group[FLAT_MAX_SEGS];     // the parameter group that owns the segment: an index into the update's hyperparameter table
};

// What every flat step refuses before it launches anything: missing tables, no segment, a group count outside [1, FLAT_MAX_GROUPS], a
// segment without elements or gradient, a segment tagged with a group that is not there.  seg_group == nullptr: every segment in group 0.
static inline bool flat_args_ok(const uint32_t* off, const uint32_t* numel, const float* const* grads, const uint8_t* seg_group, int nseg,
                                int ngroups) {
    if (!off || !numel || !grads || nseg <= 0 || ngroups < 1 || ngroups > FLAT_MAX_GROUPS) return false;
    for (int i = 0; i < nseg; ++i) {
        if (!grads[i] || numel[i] == 0) return false;
        if (seg_group && seg_group[i] >= ngroups) return false;
    }
    return true;
}

// Pack the (at most FLAT_MAX_SEGS) segments from s0 on into `a`, their tiles numbered from 0.  -> the tiles of this launch.
static inline int flat_pack(FlatSegs& a, const uint32_t* off, const uint32_t* numel, const float* const* grads, const uint8_t* seg_group,
                            int nseg, int s0) {
    a.n = nseg - s0 < FLAT_MAX_SEGS ? nseg - s0 : FLAT_MAX_SEGS;
    int tiles = 0;
    for (int i = 0; i < a.n; ++i) {
        a.tile_begin[i] = tiles;
        a.off[i] = off[s0 + i];
        a.numel[i] = numel[s0 + i];
        a.grad[i] = grads[s0 + i];
        a.group[i] = seg_group ? seg_group[s0 + i] : 0;
        tiles += (int)((numel[s0 + i] + FLAT_TILE - 1) / FLAT_TILE);
    }
    a.tile_begin[a.n] = tiles;
    return tiles;
}

// The hyperparameters of one parameter group as the kernels read them (the per-element updates of optim.hip say why these types).
struct AdamGroup {
    double lr, b1, b2, wd, eps;
    float bc1, bc2s, step;
    int decoupled;            // AdamW: the decay shrinks the parameter instead of joining the gradient
    float* step_out;          // nullable: the group's device-side step counter (state_dict)
};
struct SgdGroup {
    float wd, mom, damp1, neg_lr;      // (float)weight_decay, (float)momentum, (float)(1 - dampening), (float)(-lr)
    int wd_on, mom_on, nesterov, maximize, first;
};
struct AdamGroups { int n; AdamGroup g[FLAT_MAX_GROUPS]; };
struct SgdGroups { int n; SgdGroup g[FLAT_MAX_GROUPS]; };
static_assert(FLAT_MAX_GROUPS == MLSP_FLAT_MAX_GROUPS && FLAT_MAX_GROUPS <= 256, "seg_group is a byte per segment");
// a launch's argument block is P + FlatSegs + the update (its state pointers and group table) + tile_amax: 2576 bytes for Adam, 2344 for SGD
static_assert(sizeof(FlatSegs) == 2024 && sizeof(AdamGroups) == 520 && sizeof(SgdGroups) == 292, "kernel arguments: keep well under 4 KB");

// (both: false for a group count outside [1, FLAT_MAX_GROUPS] or a group the step cannot take; entries past n are zero)
static inline bool adam_groups_fill(AdamGroups& t, const mlsp_adam_group_t* groups, int ngroups) {
    if (!groups || ngroups < 1 || ngroups > FLAT_MAX_GROUPS) return false;
    t = AdamGroups{};
    t.n = ngroups;
    for (int i = 0; i < ngroups; ++i) {
        const mlsp_adam_group_t& q = groups[i];
        if (q.step < 1) return false;
        // (as the reference kernel: pow in double, the corrections handed on as floats)
        const float bc1 = (float)(1.0 - pow(q.beta1, (double)(float)q.step));
        const float bc2s = (float)sqrt(1.0 - pow(q.beta2, (double)(float)q.step));
        t.g[i] = AdamGroup{q.lr, q.beta1, q.beta2, q.weight_decay, q.eps, bc1, bc2s, (float)q.step, q.decoupled != 0, q.step_out};
    }
    return true;
}

static inline bool sgd_groups_fill(SgdGroups& t, const mlsp_sgd_group_t* groups, int ngroups, bool have_momentum_buffer) {
    if (!groups || ngroups < 1 || ngroups > FLAT_MAX_GROUPS) return false;
    t = SgdGroups{};
    t.n = ngroups;
    for (int i = 0; i < ngroups; ++i) {
        const mlsp_sgd_group_t& q = groups[i];
        if (q.momentum != 0.0 && !have_momentum_buffer) return false;
        // (the tests and the alphas as Python forms them: in double, then handed to the foreach ops, which take them as floats)
        t.g[i] = SgdGroup{(float)q.weight_decay, (float)q.momentum, (float)(1.0 - q.dampening), (float)(-q.lr), q.weight_decay != 0.0,
                          q.momentum != 0.0, q.nesterov != 0, q.maximize != 0, q.first != 0};
    }
    return true;
}
