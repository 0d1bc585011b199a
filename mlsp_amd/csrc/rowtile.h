// What the add-on kernel families (vecattn, gnedge, attn, token, pyramid) share: the 256-thread workgroup, the 16-byte channel quad, the
// row-tile scheme of their streaming kernels and the alignment predicate of their launchers.  No HIP runtime call: the *_body.h headers
// include it, and tools/*_host_check compile those for the host.
#pragma once
#include <stdint.h>

#define RT_HD __host__ __device__ __forceinline__
#define RT_THREADS 256
#define RT_GRID_MAX (1 << 20)

typedef float rt_f4 __attribute__((ext_vector_type(4)));
RT_HD rt_f4 rt_ld(const float* p) { return *(const rt_f4*)p; }
RT_HD void rt_st(float* p, const rt_f4& v) { *(rt_f4*)p = v; }

// rows x c4 work items (c4 channel quads per row) in tiles of `rb` rows, about 1024 items: a workgroup strides the tiles, its threads the
// items of a tile (32-bit arithmetic inside a tile, 64-bit row numbers)
struct RowTiles { int rb; long long ntiles; int grid; };
static inline RowTiles row_tiles(long long rows, int c4) {
    RowTiles t;
    t.rb = c4 >= 1024 ? 1 : 1024 / c4;
    t.ntiles = (rows + t.rb - 1) / t.rb;
    t.grid = (int)(t.ntiles < RT_GRID_MAX ? t.ntiles : RT_GRID_MAX);
    return t;
}
// the kernel side: the body sees r0_ (first row of the tile) and it_ (item in the tile: row it_ / c4, quad it_ % c4)
#define RT_FOR_ITEMS(rows_, rb_, c4_, threads_)                                                                            \
    for (long long r0_ = (long long)blockIdx.x * (rb_); r0_ < (rows_); r0_ += (long long)gridDim.x * (rb_))                \
        for (int it_ = threadIdx.x, n_ = (int)(((rows_) - r0_ < (rb_) ? (rows_) - r0_ : (long long)(rb_)) * (c4_)); it_ < n_; \
             it_ += (threads_))

// every pointer 16-byte aligned (a null pointer counts as aligned: the optional operands)
template <class... P>
static inline bool al16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }
