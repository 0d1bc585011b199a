// The reverse (transposed) neighbour index of a kNN graph or a ball-query grouping: what the backward gather-reduces of EdgeConv, set
// abstraction, propagation and vector attention walk (functional.ReverseIndex).  Not a search kernel: knn.hip / knn6.hip hold those.
#include "common.h"

// ------------------------------------------------------------------------------------------------
// Reverse neighbour index (CSR of the transposed kNN graph), one workgroup per cloud.
// For every point j: the list of (i, slot) with idx[i][slot] == j, sorted by i*256+slot so that the
// backward gather-reduce that walks it sums in a fixed order (bitwise reproducible gradients).
//   rev_off [B*N+1]  global edge offsets;  rev_ent [B*N*k]  packed (i_local << 8 | slot)
#define RV_SPLIT_MAX 16                   // workgroups per cloud: 8, or 16 when 8 would leave CUs idle (chosen by the launcher)
#define RV_CAP (16 * 1024)                // LDS entries of a slice's lists, twice: filled / ordered (a slice past that sorts in place in global memory)
// `nsplit` workgroups per cloud, each owns a contiguous slice of the destinations: it counts only the edges that point into its
// slice (LDS atomics are the expensive instruction here: ~3 clocks per lane), gets the slice's base offset by counting the edges
// that point BELOW it (plain adds + one block reduction), fills its lists and orders every list.
// pad_cnt (nullable; [B*S], from group_pad_count_kernel): the padding slots of a group -- its TRAILING run of copies of slot 0, which is
// what a ball query appends; a repeat of slot 0 further up a caller's own row is an ordinary slot -- are left out of the lists: slot s of
// group g is padding iff s >= k - pad_cnt[g].  Their rows are identical and the group's last slot is one of them, so the consumer adds
// them as a multiple of that row (sa.hip, sa_fold_bwd_point_kernel).  The lists of a cloud then no longer fill its E entries, so the
// list LENGTHS are returned as well (rev_cnt, nullable otherwise).
typedef int knn_i32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(1024) void knn_reverse_kernel(const int* __restrict__ idx, int N, int k,
                                                           int* __restrict__ rev_off, int* __restrict__ rev_ent,
                                                           int B, int S, int nsplit, const int* __restrict__ pad_cnt, int* __restrict__ rev_cnt) {
    extern __shared__ __attribute__((aligned(16))) int ism[];
    __shared__ int wsum[16];
    __shared__ int nbig;                  // lists of more than 64 entries: queued (cnt is free by then) for the whole-workgroup loop
    int b, part;
    xcd_cloud_map(blockIdx.x, nsplit, B, b, part);        // the workgroups of a cloud share an XCD (they read the same idx)
    const int tid = threadIdx.x, nt = blockDim.x;
    const int dper = (N + nsplit - 1) / nsplit, d0 = min(N, part * dper), d1 = min(N, d0 + dper), nd = d1 - d0;
    int* cnt = ism;            // [dper]
    int* off = ism + dper;     // [dper + 1]  offsets inside the slice
    int* offp = off + dper + 1;   // [dper + 1]  the same with every list padded to a multiple of 4 entries: where the lists lie in `lent`
    int* lent = ism + ((3 * dper + 2 + 3) & ~3);   // [RV_CAP] as filled; 16-byte aligned lists (pads hold INT_MAX): the ordering reads four entries per LDS instruction
    int* lord = lent + RV_CAP;    // [RV_CAP] ordered (unpadded: the slice's part of rev_ent)
    // S source rows of k slots per cloud point at N destinations (S == N for the kNN graph; the set-abstraction grouping has
    // S sampled centres gathering from N points)
    const int* ib = idx + (size_t)b * S * k;
    const int* pb = pad_cnt ? pad_cnt + (size_t)b * S : nullptr;
    const int E = S * k;
    for (int j = tid; j < nd; j += nt) cnt[j] = 0;
    if (tid == 0) nbig = 0;
    __syncthreads();
    int below = 0;
    // RV_B index loads in flight per thread (the atomics would serialise them): a pass is a chain of ceil(E / (RV_B nt)) load latencies, ONE
    // at the DGCNN shape (E = 20 Ki entries, 1024 threads) -- and then the fill pass below reuses the registers instead of reading idx again
    constexpr int RV_B = 20;
    const bool one_trip = E <= nt * RV_B;
    // Several trips (PointSegDA: N = 2048, k = 40 -> 80 entries per thread): the entries that fall into this workgroup's slice (E / nsplit of
    // them on average) are COMPACTED into `lord` as (destination, source entry) pairs while they are counted -- `lord` is free until the
    // lists are ordered -- and the fill pass walks those pairs instead of scanning the cloud's E indices again.  More than RV_CAP / 2 pairs:
    // the fill pass scans again as before.
    __shared__ int ncomp;
    if (tid == 0) ncomp = 0;
    const int comp_cap = RV_CAP / 2;
    int jk[RV_B];
    __syncthreads();
    for (int eb = tid; eb < E; eb += nt * RV_B) {
#pragma unroll
        for (int u = 0; u < RV_B; ++u) jk[u] = eb + u * nt < E ? ib[eb + u * nt] : -1;
#pragma unroll
        for (int u = 0; u < RV_B; ++u) {
            int j = jk[u];
            if (pb && j >= 0) { const int e = eb + u * nt; if (e % k >= k - pb[e / k]) j = -1; }
            jk[u] = j;
            below += j >= 0 && j < d0;
            const bool mine = j >= d0 && j < d1;
            if (mine) atomicAdd(&cnt[j - d0], 1);
            if (!one_trip) {                             // (uniform) one LDS atomic per wave and entry slot: the wave's matches take consecutive places
                const unsigned long long mm = __ballot(mine);
                if (mm) {
                    const int lane_ = tid & 63;
                    int base_ = 0;
                    if (lane_ == 0) base_ = atomicAdd(&ncomp, __builtin_popcountll(mm));
                    base_ = __shfl(base_, 0, 64);
                    const int at = base_ + __builtin_popcountll(mm & ((1ull << lane_) - 1ull));
                    if (mine && at < comp_cap) { lord[2 * at] = j - d0; lord[2 * at + 1] = eb + u * nt; }
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = below;
    __syncthreads();
    int s0 = 0;
    for (int w = 0; w < (nt >> 6); ++w) s0 += wsum[w];   // edges into the slices before this one
    // exclusive scan of the slice's counts by one wave
    if (tid < 64) {
        const int chunk = (nd + 63) / 64;
        const int beg = min(nd, tid * chunk), end = min(nd, beg + chunk);
        int sm = 0, smp = 0;
        for (int j = beg; j < end; ++j) { sm += cnt[j]; smp += (cnt[j] + 3) & ~3; }
        int incl = sm, inclp = smp;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64), tp = __shfl_up(inclp, o, 64);
            if (tid >= o) { incl += t; inclp += tp; }
        }
        int run = incl - sm, runp = inclp - smp;
        for (int j = beg; j < end; ++j) { off[j] = run; run += cnt[j]; offp[j] = runp; runp += (cnt[j] + 3) & ~3; }
        if (tid == 63) { off[nd] = incl; offp[nd] = inclp; }
    }
    __syncthreads();
    const int gbase = b * E;
    const int sn = off[nd];
    const bool in_lds = offp[nd] <= RV_CAP;
    for (int j = tid; j < nd; j += nt) {
        rev_off[(size_t)b * N + d0 + j] = gbase + s0 + off[j];
        if (rev_cnt) rev_cnt[(size_t)b * N + d0 + j] = off[j + 1] - off[j];
        if (in_lds) {
            const int c = off[j + 1] - off[j];
            for (int q = c; q < ((c + 3) & ~3); ++q) lent[offp[j] + q] = 0x7fffffff;       // pads: never below a real entry
        }
        cnt[j] = 0;
    }
    if (b == B - 1 && part == nsplit - 1 && tid == 0) rev_off[(size_t)B * N] = gbase + E;
    __syncthreads();
    // fill + order this slice's lists in LDS, then one coalesced copy out: the ordering never touches global memory
    // (a slice with more than RV_CAP entries orders in place in global memory instead)
    int* ent = in_lds ? lent : rev_ent + gbase + s0;
    const int* eoff = in_lds ? offp : off;                                 // where list j starts in `ent`
    const bool compacted = !one_trip && in_lds && ncomp <= comp_cap;       // (ncomp == sn: every pair is there)
    if (compacted) {
        for (int i = tid; i < sn; i += nt) {
            const int jl = lord[2 * i], e = lord[2 * i + 1];
            const int pos = atomicAdd(&cnt[jl], 1);
            ent[eoff[jl] + pos] = ((e / k) << 8) | (e % k);
        }
    } else
    for (int eb = tid; eb < E; eb += nt * RV_B) {
        if (!one_trip) {
#pragma unroll
            for (int u = 0; u < RV_B; ++u) jk[u] = eb + u * nt < E ? ib[eb + u * nt] : -1;
        }
#pragma unroll
        for (int u = 0; u < RV_B; ++u) {
            int j = jk[u];
            const int e = eb + u * nt;
            if (!one_trip && pb && j >= 0 && e % k >= k - pb[e / k]) j = -1;
            if (j >= d0 && j < d1) {
                const int pos = atomicAdd(&cnt[j - d0], 1);
                ent[eoff[j - d0] + pos] = ((e / k) << 8) | (e % k);
            }
        }
    }
    __syncthreads();
    if (in_lds) {
        // order every list by (i, slot) by RANK: 16 lanes per list, every lane ranks its entries against the whole list (the 16 lanes
        // read the same LDS words: broadcasts) and writes them straight to their final place.  Lists of more than 64 entries
        // (ball-query groups are padded with copies of their first hit: a few points collect hundreds of edges) are left to the
        // second loop, where the whole workgroup shares one list.
        int* out = lord;
        const int lg = tid >> 4, ll = tid & 15;
        for (int j = lg; j < nd; j += nt >> 4) {
            const int e0 = off[j], n = off[j + 1] - e0;
            if (n > 64) {
                if (ll == 0) cnt[atomicAdd(&nbig, 1)] = j;
                continue;
            }
            const int* a = ent + offp[j];                  // 16-byte aligned, padded with INT_MAX to a multiple of 4
            for (int q = ll; q < n; q += 16) {
                const int v = a[q];
                int rank = 0;
                for (int e = 0; e < n; e += 4) {
                    const knn_i32x4 t = *(const knn_i32x4*)(a + e);
                    rank += (t[0] < v) + (t[1] < v) + (t[2] < v) + (t[3] < v);
                }
                out[e0 + rank] = v;
            }
        }
        __syncthreads();
        // lists of 65 .. 512 entries (the tail of a kNN graph's in-degree distribution: a dozen per workgroup at k = 40, a few at k = 20):
        // ONE WAVE per list, sixteen lists at a time -- the whole workgroup walking them one after the other was the longest phase of the
        // kernel (8 of 21 us at k = 20, 29 of 61 us at k = 40, N = 2048).  Longer ones (ball-query hubs): the whole workgroup per list.
        {
            const int wv = tid >> 6, ln = tid & 63;
            for (int bi = wv; bi < nbig; bi += nt >> 6) {
                const int j = cnt[bi];
                const int e0 = off[j], n = off[j + 1] - e0;
                if (n > 512) continue;
                const int* a = ent + offp[j];
                for (int q = ln; q < n; q += 64) {
                    const int v = a[q];
                    int rank = 0;
                    for (int e = 0; e < n; e += 4) {
                        const knn_i32x4 t = *(const knn_i32x4*)(a + e);
                        rank += (t[0] < v) + (t[1] < v) + (t[2] < v) + (t[3] < v);
                    }
                    out[e0 + rank] = v;
                }
            }
        }
        for (int bi = 0; bi < nbig; ++bi) {
            const int j = cnt[bi];
            const int e0 = off[j], n = off[j + 1] - e0;
            if (n <= 512) continue;
            const int* a = ent + offp[j];
            for (int q = tid; q < n; q += nt) {
                const int v = a[q];
                int rank = 0;
                for (int e = 0; e < n; ++e) rank += a[e] < v;
                out[e0 + rank] = v;
            }
        }
        __syncthreads();
        for (int i = tid; i < sn; i += nt) rev_ent[gbase + s0 + i] = lord[i];      // one coalesced copy out
        return;
    }
    __threadfence_block();
    // a slice too large for LDS: per-destination insertion sort in place in global memory
    for (int j = tid; j < nd; j += nt) {
        int* a = ent + off[j];
        const int n = off[j + 1] - off[j];
        for (int u = 1; u < n; ++u) {
            const int key = a[u];
            int w = u - 1;
            while (w >= 0 && a[w] > key) { a[w + 1] = a[w]; --w; }
            a[w + 1] = key;
        }
    }
}

// pad_cnt [B*S] = number of padding slots of every group: the length of the trailing run of slots s > 0 with idx[i][s] == idx[i][0]
// (0 .. k - 1).  Counted BEFORE the lists are built: knn_reverse_kernel reads it, so both hold ONE definition of a padding slot and
// "pad_cnt times the row of the last slot" is right for any idx, not only for the trailing pads a ball query makes.
__global__ __launch_bounds__(256) void group_pad_count_kernel(const int* __restrict__ idx, int G, int k, int* __restrict__ pad_cnt) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int* r = idx + (size_t)g * k;
    const int first = r[0];
    int c = 0;
    for (int s = 1; s < k; ++s) c = r[s] == first ? c + 1 : 0;      // (a forward pass over independent loads: the run that reaches slot k - 1)
    pad_cnt[g] = c;
}

// pad_cnt / rev_cnt: both or neither (the compact form)
static int launch_reverse(hipStream_t st, const int* idx, int B, int S, int N, int k, int* rev_off, int* rev_ent, int* pad_cnt = nullptr,
                          int* rev_cnt = nullptr) {
    if (!idx || !rev_off || !rev_ent || B <= 0 || N <= 0 || S <= 0 || k <= 0 || k > 256 || N > (1 << 22) || S > (1 << 22)) return MLSP_ERR_ARG;
    const int nsplit = B * 8 >= 256 || N < 1024 ? 8 : RV_SPLIT_MAX;
    const int dper = (N + nsplit - 1) / nsplit;
    const size_t lds = (size_t)(((3 * dper + 2 + 3) & ~3) + 2 * RV_CAP) * sizeof(int);
    if (lds > 160 * 1024) return MLSP_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        hipError_t e = mlsp_lds_limit((const void*)knn_reverse_kernel, lds);
        if (e != hipSuccess) return (int)e;
    }
    if (pad_cnt) hipLaunchKernelGGL(group_pad_count_kernel, dim3((B * S + 255) / 256), dim3(256), 0, st, idx, B * S, k, pad_cnt);
    hipLaunchKernelGGL(knn_reverse_kernel, dim3(B * nsplit), dim3(1024), lds, st, idx, N, k, rev_off, rev_ent, B, S, nsplit, (const int*)pad_cnt, rev_cnt);
    return mlsp_launch_status();
}

// ball-query groups (padded with copies of the first hit)
int launch_group_reverse(hipStream_t st, const int* idx, int B, int S, int N, int k, int* rev_off, int* rev_ent) {
    return launch_reverse(st, idx, B, S, N, k, rev_off, rev_ent);
}
// the same without the padding slots (the trailing copies of slot 0), and how many each group has
int launch_group_reverse_compact(hipStream_t st, const int* idx, int B, int S, int N, int k, int* rev_off, int* rev_cnt, int* rev_ent,
                                 int* pad_cnt) {
    if (!rev_cnt || !pad_cnt) return MLSP_ERR_ARG;
    return launch_reverse(st, idx, B, S, N, k, rev_off, rev_ent, pad_cnt, rev_cnt);
}
int launch_knn_reverse(hipStream_t st, const int* idx, int B, int N, int k, int* rev_off, int* rev_ent) {
    return launch_reverse(st, idx, B, N, N, k, rev_off, rev_ent);
}
