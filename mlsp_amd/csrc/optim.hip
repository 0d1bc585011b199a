// Optimizer steps of the hot path.  Adam (PointDA/trainer.py:258-259: optim.Adam(model.parameters(), lr, weight_decay), stepped at :571) over FLAT
// parameter / moment buffers in one launch.
//
// torch's fused Adam hands every workgroup one 64 Ki-element chunk of one tensor: 4.55 M parameters are 70-odd mostly full chunks plus 77
// tails, i.e. a quarter of the chip moving 127 MB -- 110 us in five launches (profiles/r5_*).  Here the parameters, exp_avg and exp_avg_sq
// live in three flat fp32 buffers (mlsp_amd/optim.py), the gradients are read WHERE AUTOGRAD LEFT THEM through a pointer table in the
// kernel arguments (no packing copy), and a workgroup owns a 2048-element tile: ~2300 workgroups, one pass at the HBM roof.
//
// Arithmetic: the element-wise update of torch's fused kernel (ATen/native/cuda/fused_adam_utils.cuh `adam_math`, ADAM_MODE::ORIGINAL, no
// amsgrad / maximize / grad scaling), restated with its types: lr, beta1, beta2, weight_decay, eps are doubles there, so the products with
// them are formed in double and rounded to float on assignment; the two bias corrections are rounded to float before use.
//   grad   += param * weight_decay                          (double, float result)
//   exp_avg = beta1 * exp_avg + (1 - beta1) * grad          (double)
//   exp_avg_sq = beta2 * exp_avg_sq + (1 - beta2) * grad * grad   (double, left to right)
//   step_size = lr / bias_correction1 ;  denom = sqrt(exp_avg_sq) / bias_correction2_sqrt + eps ;  param -= step_size * exp_avg / denom
// The one freedom the source leaves is the lowering: torch's build contracts each double a * b + c above into an fma and keeps the float
// division and square root correctly rounded -- established by tools/r5/adam_probe (32 lowerings against torch._fused_adam_ on 4 Mi
// elements: this one differs in 0 elements of param / exp_avg / exp_avg_sq, the uncontracted form in 16,285 exp_avg values;
// profiles/r5_adam_lowering_probe.txt).  This file is compiled with -ffp-contract=off, so the fmas are written out.
// tests/test_gpu_optim.py asserts bit-identity with torch.optim.Adam(fused=True) step by step.
//
// AdamW (ADAM_MODE::ADAMW, torch.optim.AdamW = Adam(decoupled_weight_decay=True)): nothing joins the gradient; before the moments
//   param -= lr * weight_decay * param                      (double: (lr * weight_decay) * param, float result)
// written as one fma like every other double a * b + c of the update.  tools/adamw_probe (against torch._fused_adamw_ on 4 Mi elements,
// profiles/adamw_lowering_probe.txt) finds 0 differing elements for the fma AND for the uncontracted form: they part only where the
// product's rounding in double, 29 bits below the float result's last place, decides a near-tie.
//
// Parameter groups: a segment carries the index of its group (FlatSegs::group, a byte), the update carries a table of up to
// FLAT_MAX_GROUPS = 8 hyperparameter entries (AdamGroups / SgdGroups, flat_segs.h), and a workgroup reads the entry of the segment that owns
// its tile -- a workgroup-uniform lookup after the segment search.  Kernel arguments: P (8) + FlatSegs (2024, was 1928) + AdamUpdate (536) |
// SgdUpdate (304) + tile_amax (8) = 2576 | 2344 bytes of the 4096 a launch may carry.  tests/test_gpu_optim_groups.py asserts bit-identity
// with torch's optimizers over several groups step by step.
//
// SGD step (the trainers' --optimizer SGD) over a flat parameter buffer and a flat momentum buffer: the same tiles, segment lookup, gradient
// table and tile_amax epilogue (flat_step_tile, templated on the per-element update), the arithmetic of torch's default multi-tensor SGD
// (SgdUpdate below).  tests/test_gpu_optim_sgd.py asserts bit-identity with torch.optim.SGD step by step.
#include "common.h"
#include "flat_segs.h"

__device__ __forceinline__ void adam_one(float& param, float grad, float& ea, float& es, const AdamGroup& h) {
    if (h.wd != 0.0) {
        if (h.decoupled) param = (float)fma(-(h.lr * h.wd), (double)param, (double)param);
        else grad = (float)fma((double)param, h.wd, (double)grad);
    }
    ea = (float)fma(h.b1, (double)ea, (1.0 - h.b1) * (double)grad);
    es = (float)fma(h.b2, (double)es, ((1.0 - h.b2) * (double)grad) * (double)grad);
    const float step_size = (float)(h.lr / (double)h.bc1);
    const float denom = (float)((double)(sqrtf(es) / h.bc2s) + h.eps);
    param -= step_size * ea / denom;
}

// The per-element update of one optimizer over the flat buffers.  group(gi) is the hyperparameter entry of parameter group gi (the caller
// passes a workgroup-uniform index: scalar loads from the kernel arguments); one4 updates four parameters at flat element k (16-byte aligned)
// with their gradients under that entry, one1 a single parameter; both read and write the optimizer's own state streams at the same element.
struct AdamUpdate {
    typedef AdamGroup Group;
    float* M;                 // exp_avg
    float* V;                 // exp_avg_sq
    AdamGroups t;
    __device__ __forceinline__ void begin(int tile) const {
        if (tile == 0 && threadIdx.x == 0)
            for (int i = 0; i < t.n; ++i)
                if (t.g[i].step_out) *t.g[i].step_out = t.g[i].step;
    }
    __device__ __forceinline__ Group group(int gi) const { return t.g[gi]; }
    __device__ __forceinline__ void one4(const Group& h, f32x4& pp, const f32x4& gg, unsigned k) const {
        f32x4 mm = *(const f32x4*)(M + k), vv = *(const f32x4*)(V + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float p1 = pp[e], m1 = mm[e], v1 = vv[e];
            adam_one(p1, gg[e], m1, v1, h);
            pp[e] = p1; mm[e] = m1; vv[e] = v1;
        }
        *(f32x4*)(M + k) = mm; *(f32x4*)(V + k) = vv;
    }
    __device__ __forceinline__ void one1(const Group& h, float& pp, float g, unsigned k) const {
        float mm = M[k], vv = V[k];
        adam_one(pp, g, mm, vv, h);
        M[k] = mm; V[k] = vv;
    }
};

// torch.optim.SGD's default path on GPU tensors (torch/optim/sgd.py _multi_tensor_sgd) restated type by type: each foreach op rounds its
// float result, every scalar reaches it as a float alpha, and each `a + alpha * b` of torch's ROCm build is one fma (tools/sgd_probe,
// profiles/sgd_lowering_probe.txt).  torch steps group after group, so every group brings its own scalars and its own `first`.
struct SgdUpdate {
    typedef SgdGroup Group;
    float* B;                 // momentum_buffer (unused by a group with !mom_on)
    SgdGroups t;
    __device__ __forceinline__ void begin(int) const {}
    __device__ __forceinline__ Group group(int gi) const { return t.g[gi]; }
    static __device__ __forceinline__ float grad(const Group& h, float param, float g) {
        if (h.maximize) g = -g;                                 // _foreach_neg(grads)
        if (h.wd_on) g = fmaf(h.wd, param, g);                  // _foreach_add(grads, params, alpha=weight_decay)
        return g;
    }
    static __device__ __forceinline__ float with_momentum(const Group& h, float g, float& buf) {
        buf = h.first ? g : fmaf(h.damp1, g, buf * h.mom);     // clone(grad) | _foreach_mul_(bufs, momentum); _foreach_add_(bufs, grads, alpha=1 - dampening)
        return h.nesterov ? fmaf(h.mom, buf, g) : buf;          // _foreach_add_(grads, bufs, alpha=momentum) | grads = bufs
    }
    __device__ __forceinline__ void one4(const Group& h, f32x4& pp, const f32x4& gg, unsigned k) const {
        if (h.mom_on) {
            f32x4 bb = h.first ? f32x4{} : *(const f32x4*)(B + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float b1 = bb[e];
                const float d = with_momentum(h, grad(h, pp[e], gg[e]), b1);
                bb[e] = b1;
                pp[e] = fmaf(h.neg_lr, d, pp[e]);               // _foreach_add_(params, grads, alpha=-lr)
            }
            *(f32x4*)(B + k) = bb;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) pp[e] = fmaf(h.neg_lr, grad(h, pp[e], gg[e]), pp[e]);
        }
    }
    __device__ __forceinline__ void one1(const Group& h, float& pp, float g, unsigned k) const {
        float d = grad(h, pp, g);
        if (h.mom_on) {
            float b1 = h.first ? 0.f : B[k];
            d = with_momentum(h, d, b1);
            B[k] = b1;
        }
        pp = fmaf(h.neg_lr, d, pp);
    }
};

// One 2048-element tile of the flat parameter buffer P per workgroup, whatever the optimizer: find the segment that owns the tile, fetch the
// hyperparameters of the segment's parameter group, update the tile's parameters (16 bytes per lane where the segment's offset and gradient
// allow), and leave the tile's largest updated magnitude.
template <class Update>
__device__ __forceinline__ void flat_step_tile(float* __restrict__ P, const FlatSegs& s, const Update& up, float* __restrict__ tile_amax) {
    // tile_amax (nullable, [gridDim.x]): max |updated parameter| of this workgroup's tile -- a by-product for the GEMMs that read the
    // parameters next (the two-piece f16 products scale every operand by a bound of its magnitude: include/mlsp_hip.h mlsp_bound_t)
    float pmx = 0.f;
    const int t = blockIdx.x;
    up.begin(t);
    // which segment owns this tile: binary search over <= 96 tile offsets in the kernel arguments
    int lo = 0, hi = s.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s.tile_begin[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const unsigned n = s.numel[lo];
    const unsigned base = s.off[lo];
    const unsigned e0 = (unsigned)(t - s.tile_begin[lo]) * FLAT_TILE;
    const float* __restrict__ g = s.grad[lo];
    // (the owning group is the same for every lane: the index goes through a scalar register, the entry is read with scalar loads)
    const typename Update::Group h = up.group(__builtin_amdgcn_readfirstlane((int)s.group[lo]));
    float* p = P + base;
    const bool gvec = (((uintptr_t)g) & 15) == 0 && (base & 3) == 0;      // 16-byte accesses on every stream
#pragma unroll
    for (int u = 0; u < FLAT_TILE / 1024; ++u) {
        const unsigned i = e0 + u * 1024 + threadIdx.x * 4;
        if (i >= n) break;
        if (i + 4 <= n && gvec) {
            f32x4 pp = *(const f32x4*)(p + i);
            const f32x4 gg = *(const f32x4*)(g + i);
            up.one4(h, pp, gg, base + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) pmx = fmaxf(pmx, fabsf(pp[e]));
            *(f32x4*)(p + i) = pp;
        } else {
            for (unsigned j = i; j < n && j < i + 4; ++j) {
                float pp = p[j];
                up.one1(h, pp, g[j], base + j);
                p[j] = pp;
                pmx = fmaxf(pmx, fabsf(pp));
            }
        }
    }
    if (tile_amax) {                    // (uniform: a kernel argument)
        __shared__ float smx[4];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pmx = fmaxf(pmx, __shfl_xor(pmx, o, 64));
        if ((threadIdx.x & 63) == 0) smx[threadIdx.x >> 6] = pmx;
        __syncthreads();
        if (threadIdx.x == 0) tile_amax[t] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
    }
}

// (one named kernel per optimizer: the names are what kernel traces show)
__global__ __launch_bounds__(256) void adam_flat_kernel(float* __restrict__ P, FlatSegs s, AdamUpdate up, float* __restrict__ tile_amax) {
    flat_step_tile(P, s, up, tile_amax);
}

__global__ __launch_bounds__(256) void sgd_flat_kernel(float* __restrict__ P, FlatSegs s, SgdUpdate up, float* __restrict__ tile_amax) {
    flat_step_tile(P, s, up, tile_amax);
}

// Launch `kernel` over nseg segments in chunks of 96, tiles numbered segment by segment across the chunks (tile_amax); every chunk carries the
// whole group table of `up`.  Nothing is launched unless every segment passes flat_args_ok.
template <class Update>
static int flat_launch(void (*kernel)(float*, FlatSegs, Update, float*), float* P, const uint32_t* off, const uint32_t* numel,
                       const float* const* grads, const uint8_t* seg_group, int nseg, const Update& up, float* tile_amax, mlsp_stream_t st) {
    if (!flat_args_ok(off, numel, grads, seg_group, nseg, up.t.n)) return MLSP_ERR_ARG;
    size_t tile_base = 0;
    for (int s0 = 0; s0 < nseg; s0 += FLAT_MAX_SEGS) {
        FlatSegs a;
        const int tiles = flat_pack(a, off, numel, grads, seg_group, nseg, s0);
        hipLaunchKernelGGL(kernel, dim3(tiles), dim3(256), 0, st, P, a, up, tile_amax ? tile_amax + tile_base : (float*)nullptr);
        tile_base += tiles;
    }
    return mlsp_launch_status();
}

static bool aligned16(const void* a, const void* b = nullptr, const void* c = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

extern "C" {

// One Adam / AdamW step over nseg parameter segments of the flat buffers P / M / V (exp_avg / exp_avg_sq): segment s covers elements
// [off[s], off[s] + numel[s]) (the buffers 16-byte aligned; a segment whose offset and gradient pointer are 16-byte aligned moves 16 bytes per
// lane, any other one element by element), reads its gradient from grads[s] (any fp32 device pointer, contiguous) and steps with the
// hyperparameters of groups[seg_group[s]] (seg_group nullable: group 0).  A group's step >= 1 is this update's number for its parameters
// (bias corrections 1 - beta^step); its step_out (nullable, device float) receives it.  Host arrays; any nseg (launched in chunks of 96).
// tile_amax (nullable; ABI v13): one float per 2048-element tile, tiles numbered segment by segment in the order given
// (ceil(numel[s] / 2048) tiles per segment): the largest magnitude of the UPDATED parameters of the tile.
int mlsp_adam_flat_groups_f32(float* P, float* M, float* V, const uint32_t* off, const uint32_t* numel, const float* const* grads,
                              const uint8_t* seg_group, int nseg, const mlsp_adam_group_t* groups, int ngroups, float* tile_amax,
                              mlsp_stream_t st) {
    if (!P || !M || !V || !aligned16(P, M, V)) return MLSP_ERR_ARG;
    AdamUpdate up{M, V, {}};
    if (!adam_groups_fill(up.t, groups, ngroups)) return MLSP_ERR_ARG;
    return flat_launch(adam_flat_kernel, P, off, numel, grads, seg_group, nseg, up, tile_amax, st);
}

// The one-group form: torch.optim.Adam's coupled weight decay.
int mlsp_adam_flat_f32(float* P, float* M, float* V, const uint32_t* off, const uint32_t* numel, const float* const* grads, int nseg, double lr,
                       double beta1, double beta2, double weight_decay, double eps, int64_t step, float* step_out, float* tile_amax,
                       mlsp_stream_t st) {
    const mlsp_adam_group_t g{lr, beta1, beta2, weight_decay, eps, step, 0, step_out};
    return mlsp_adam_flat_groups_f32(P, M, V, off, numel, grads, nullptr, nseg, &g, 1, tile_amax, st);
}

// One SGD step (torch.optim.SGD; PointDA/trainer.py:258-259 with --optimizer SGD) over the flat parameter buffer P and momentum buffer B
// (nullable when every group has momentum == 0), segments, gradients and groups as mlsp_adam_flat_groups_f32.  A group's first != 0: its
// part of B is initialised with the gradient (torch's first step, where momentum_buffer is a clone) instead of updated.
int mlsp_sgd_flat_groups_f32(float* P, float* B, const uint32_t* off, const uint32_t* numel, const float* const* grads, const uint8_t* seg_group,
                             int nseg, const mlsp_sgd_group_t* groups, int ngroups, float* tile_amax, mlsp_stream_t st) {
    if (!P || !aligned16(P, B)) return MLSP_ERR_ARG;
    SgdUpdate up{B, {}};
    if (!sgd_groups_fill(up.t, groups, ngroups, B != nullptr)) return MLSP_ERR_ARG;
    return flat_launch(sgd_flat_kernel, P, off, numel, grads, seg_group, nseg, up, tile_amax, st);
}

int mlsp_sgd_flat_f32(float* P, float* B, const uint32_t* off, const uint32_t* numel, const float* const* grads, int nseg, double lr,
                      double momentum, double dampening, double weight_decay, int nesterov, int maximize, int first, float* tile_amax,
                      mlsp_stream_t st) {
    const mlsp_sgd_group_t g{lr, momentum, dampening, weight_decay, nesterov, maximize, first};
    return mlsp_sgd_flat_groups_f32(P, B, off, numel, grads, nullptr, nseg, &g, 1, tile_amax, st);
}

}  // extern "C"
