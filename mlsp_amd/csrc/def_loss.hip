// The index-matched losses on the deformed region (MLSP/mlsp.py:184-220, 289-427):
//   findindexs / findneareat_index   :184-220   nearest gold point of every predicted point and the reverse (+100 on unmasked columns)
//   calc_def_normal_loss             :289-329   |cos| normal loss matched through both index sets
//   deform_densityloss               :370-427   two densityloss (:430-454) evaluations matched through both index sets
//   calc_def_density_loss            :331-368   a caller-supplied criterion: only its row gathers are kernels here
// Unlike chamfer_dir_fwd_kernel (loss.hip), which scans the ~N/27 masked rows, every row of both clouds is searched.
// Backward passes scatter through index2 with a per-cloud grouping built in LDS (bitonic sort of index*NP + j): every sum runs in
// a fixed order (ascending j, or a fixed lane stride + shuffle tree for long rows), so gradients are bit-identical run to run
// without float atomics.
// Bounds: 1 <= N <= DEF_MAX_N (LDS: 16 N bytes for the search, 8 N bytes for the grouping).  An index outside [0, N) is never
// dereferenced: its row contributes zero (gather: writes zero).
#include "common.h"
#include <math.h>
#include <limits.h>

#define DEF_MAX_N 4096
#define DEF_PARTS 256

static inline int def_pow2(int n) {
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// mask_cord of calc_def_normal_loss / deform_densityloss (:291-295, :373-377): m if Density_normal_defpart else 26 m + 1
__device__ __forceinline__ float def_weight(float m, int defpart) { return defpart ? m : m * 26.f + 1.f; }

__device__ __forceinline__ bool def_valid(int64_t t, int N) { return t >= 0 && t < N; }

// ---------------------------------------------------------------------------------------------
// index1[b][i] = argmin_j |pred_bi - gold_bj|^2 + pen_bj ; index2[b][j] = argmin_i |gold_bj - pred_bi|^2 + pen_bi
// pen_j = 100 if mask[b][0][j] == 0, 0 if it is 1, the mask value otherwise (the m[m==0]=100; m[m==1]=0 of :212-214).
// pred [B][N][3], gold [B][3][N], mask [B][3][N].  Grid (row blocks, B, 2 directions); one thread per row walks all columns of the
// other cloud in ascending order from LDS (a broadcast read), strict < keeps the lowest j on ties as torch.min does.  Distance as
// the reference's torch.norm(...)**2 (:205-206) in fp32: ((dx^2 + dy^2) + dz^2), sqrt, squared (the build has -ffp-contract=off).
__global__ __launch_bounds__(256) void def_nearest_kernel(const float* __restrict__ pred, const float* __restrict__ gold,
                                                          const float* __restrict__ mask, int N, int64_t* __restrict__ index1,
                                                          int64_t* __restrict__ index2) {
    extern __shared__ f32x4 ncol[];   // columns {x, y, z, penalty} [N]
    const int b = blockIdx.y, dir = blockIdx.z, tid = threadIdx.x;
    const float* pb = pred + (size_t)b * N * 3;
    const float* gb = gold + (size_t)b * 3 * N;
    const float* mb = mask + (size_t)b * 3 * N;
    for (int n = tid; n < N; n += blockDim.x) {
        const float m = mb[n];
        f32x4 c;
        if (dir == 0) { c.x = gb[n]; c.y = gb[N + n]; c.z = gb[2 * N + n]; }
        else { c.x = pb[n * 3]; c.y = pb[n * 3 + 1]; c.z = pb[n * 3 + 2]; }
        c.w = m == 0.f ? 100.f : (m == 1.f ? 0.f : m);
        ncol[n] = c;
    }
    __syncthreads();
    const int i = blockIdx.x * blockDim.x + tid;
    if (i >= N) return;
    float ax, ay, az;
    if (dir == 0) { ax = pb[i * 3]; ay = pb[i * 3 + 1]; az = pb[i * 3 + 2]; }
    else { ax = gb[i]; ay = gb[N + i]; az = gb[2 * N + i]; }
    float best = INFINITY;
    int bj = 0;
#pragma unroll 4
    for (int j = 0; j < N; ++j) {
        const f32x4 c = ncol[j];
        const float dx = ax - c.x, dy = ay - c.y, dz = az - c.z;
        const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
        const float d = nrm * nrm + c.w;
        if (d < best) { best = d; bj = j; }
    }
    (dir == 0 ? index1 : index2)[(size_t)b * N + i] = bj;
}

// ---------------------------------------------------------------------------------------------
// Per-cloud reverse grouping of an index row idx[0..N): afterwards the j with idx[j] == i are keys[seg[i] .. seg[i+1]) & (NP-1), in
// ascending j.  keys [NP] (NP = next power of two >= N), seg [N+1], both LDS.  Ends with a barrier.
__device__ void def_group(const int64_t* __restrict__ idx, int N, int NP, int* keys, int* seg) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int j = tid; j < NP; j += nt) {
        int k = INT_MAX;
        if (j < N) {
            const int64_t t = idx[j];
            if (def_valid(t, N)) k = (int)t * NP + j;
        }
        keys[j] = k;
    }
    __syncthreads();
    for (int k = 2; k <= NP; k <<= 1)
        for (int s = k >> 1; s > 0; s >>= 1) {
            for (int t = tid; t < (NP >> 1); t += nt) {
                const int a = (t / s) * 2 * s + (t % s), c = a + s;
                const int ka = keys[a], kc = keys[c];
                if ((ka > kc) == ((a & k) == 0)) { keys[a] = kc; keys[c] = ka; }
            }
            __syncthreads();
        }
    for (int r = tid; r <= N; r += nt) {   // first position with key >= r * NP
        const int target = r * NP;
        int lo = 0, hi = NP;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < target) lo = mid + 1; else hi = mid;
        }
        seg[r] = lo;
    }
    __syncthreads();
}

// Rows with more than DEF_SHORT contributors (index2 piles the unmasked gold points onto the few dozen masked predictions: the
// +100 penalty) are summed by a whole wave -- lanes stride the row's segment, then a fixed shuffle tree; shorter rows stay one thread
// per row.  Both orders are fixed, so the result is the same bits on every run.
#define DEF_SHORT 4

__device__ __forceinline__ float def_wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void def_block_sum3(double& a, double& b, double& c, double* sh) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); c += __shfl_xor(c, o, 64);
    }
    if (lane == 0) { sh[w * 3] = a; sh[w * 3 + 1] = b; sh[w * 3 + 2] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double x = 0, y = 0, z = 0;
        for (int u = 0; u < (int)(blockDim.x >> 6); ++u) { x += sh[u * 3]; y += sh[u * 3 + 1]; z += sh[u * 3 + 2]; }
        a = x; b = y; c = z;
    }
}

// F.normalize(v, p=2, dim=-1) (eps 1e-12); returns the clamped norm
__device__ __forceinline__ float def_unit(const float* v, float* u) {
    const float n = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-12f);
    u[0] = v[0] / n; u[1] = v[1] / n; u[2] = v[2] / n;
    return n;
}

// normal loss partials, one workgroup per cloud: part[b] = {sum_i w_i |ph_i . gh_idx1(i)| + sum_j w_j |ph_idx2(j) . gh_j|, sum w}
__global__ __launch_bounds__(256) void def_normal_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ lab,
                                                             const float* __restrict__ mask, const int64_t* __restrict__ index1,
                                                             const int64_t* __restrict__ index2, int N, int defpart,
                                                             double* __restrict__ part) {
    __shared__ double sh[12];
    const int b = blockIdx.x;
    const float* pb = pred + (size_t)b * N * 3;
    const float* lb = lab + (size_t)b * N * 3;
    double s = 0.0, sw = 0.0, dummy = 0.0;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const float w = def_weight(mask[(size_t)b * 3 * N + i], defpart);
        float u[3], v[3], c1 = 0.f, c2 = 0.f;
        const int64_t t1 = index1[(size_t)b * N + i], t2 = index2[(size_t)b * N + i];
        if (def_valid(t1, N)) {
            def_unit(pb + i * 3, u); def_unit(lb + t1 * 3, v);
            c1 = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
        }
        if (def_valid(t2, N)) {
            def_unit(pb + t2 * 3, u); def_unit(lb + i * 3, v);
            c2 = u[0] * v[0] + u[1] * v[1] + u[2] * v[2];
        }
        s += (double)(fabsf(c1) * w) + (double)(fabsf(c2) * w);
        sw += w;
    }
    def_block_sum3(s, sw, dummy, sh);
    if (threadIdx.x == 0) { part[b * 2] = s; part[b * 2 + 1] = sw; }
}

// out[0] = -weight / B * sum_b S_b / W_b ; out[1 + b] = W_b (kept for the backward)
__global__ __launch_bounds__(64) void def_normal_finalize_kernel(const double* __restrict__ part, int B, float weight,
                                                                 float* __restrict__ out) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < B; ++b) { s += part[b * 2] / part[b * 2 + 1]; out[1 + b] = (float)part[b * 2 + 1]; }
        out[0] = (float)(-(double)weight * s / B);
    }
}

// dpred_bi = coef_b / |p_bi| * [ w_i sg1 (gh_idx1(i) - c1 ph_i) + sum_{j: idx2(j) = i} w_j sg2_j (gh_j - c2_j ph_i) ],
// coef_b = -g * weight / (B W_b).  One workgroup per cloud.
__global__ __launch_bounds__(1024) void def_normal_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ lab,
                                                              const float* __restrict__ mask, const int64_t* __restrict__ index1,
                                                              const int64_t* __restrict__ index2, int B, int N, int NP, int defpart,
                                                              float weight, const float* __restrict__ fwd_out,
                                                              const float* __restrict__ gout, float* __restrict__ dpred) {
    extern __shared__ int gsm[];
    int* keys = gsm;
    int* seg = gsm + NP;
    const int b = blockIdx.x;
    def_group(index2 + (size_t)b * N, N, NP, keys, seg);
    const float* pb = pred + (size_t)b * N * 3;
    const float* lb = lab + (size_t)b * N * 3;
    const float* mb = mask + (size_t)b * 3 * N;
    const float coef = -gout[0] * weight / ((float)B * fwd_out[1 + b]);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        if (seg[i + 1] - seg[i] > DEF_SHORT) continue;          // a wave takes it below
        float ph[3], gh[3];
        const float np = def_unit(pb + i * 3, ph);
        float ax = 0.f, ay = 0.f, az = 0.f;
        const int64_t t1 = index1[(size_t)b * N + i];
        if (def_valid(t1, N)) {
            def_unit(lb + t1 * 3, gh);
            const float c = ph[0] * gh[0] + ph[1] * gh[1] + ph[2] * gh[2];
            const float f = def_weight(mb[i], defpart) * (float)((c > 0.f) - (c < 0.f));
            ax += f * (gh[0] - c * ph[0]); ay += f * (gh[1] - c * ph[1]); az += f * (gh[2] - c * ph[2]);
        }
        for (int q = seg[i]; q < seg[i + 1]; ++q) {
            const int j = keys[q] & (NP - 1);
            def_unit(lb + j * 3, gh);
            const float c = ph[0] * gh[0] + ph[1] * gh[1] + ph[2] * gh[2];
            const float f = def_weight(mb[j], defpart) * (float)((c > 0.f) - (c < 0.f));
            ax += f * (gh[0] - c * ph[0]); ay += f * (gh[1] - c * ph[1]); az += f * (gh[2] - c * ph[2]);
        }
        const float k = coef / np;
        float* o = dpred + ((size_t)b * N + i) * 3;
        o[0] = k * ax; o[1] = k * ay; o[2] = k * az;
    }
    for (int r0 = wave * 64; r0 < N; r0 += nw * 64) {
        const int ri = r0 + lane;
        unsigned long long todo = __ballot(ri < N && seg[ri + 1] - seg[ri] > DEF_SHORT);
        while (todo) {
            const int i = r0 + __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            float ph[3], gh[3];
            const float np = def_unit(pb + i * 3, ph);
            float ax = 0.f, ay = 0.f, az = 0.f;
            for (int q = seg[i] + lane; q < seg[i + 1]; q += 64) {
                const int j = keys[q] & (NP - 1);
                def_unit(lb + j * 3, gh);
                const float c = ph[0] * gh[0] + ph[1] * gh[1] + ph[2] * gh[2];
                const float f = def_weight(mb[j], defpart) * (float)((c > 0.f) - (c < 0.f));
                ax += f * (gh[0] - c * ph[0]); ay += f * (gh[1] - c * ph[1]); az += f * (gh[2] - c * ph[2]);
            }
            ax = def_wave_sum(ax); ay = def_wave_sum(ay); az = def_wave_sum(az);
            if (lane == 0) {
                const int64_t t1 = index1[(size_t)b * N + i];
                if (def_valid(t1, N)) {
                    def_unit(lb + t1 * 3, gh);
                    const float c = ph[0] * gh[0] + ph[1] * gh[1] + ph[2] * gh[2];
                    const float f = def_weight(mb[i], defpart) * (float)((c > 0.f) - (c < 0.f));
                    ax += f * (gh[0] - c * ph[0]); ay += f * (gh[1] - c * ph[1]); az += f * (gh[2] - c * ph[2]);
                }
                const float k = coef / np;
                float* o = dpred + ((size_t)b * N + i) * 3;
                o[0] = k * ax; o[1] = k * ay; o[2] = k * az;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// deform_densityloss partials over all B*N rows r = (b, i), t1 = b*N + idx1(r), t2 = b*N + idx2(r):
//   a  += w_r [ sum_c lvec[t1][c] log(pvec[r][c] + 1e-10) + sum_c pvec[t2][c] log(lvec[r][c] + 1e-10) ]
//   e  += w_r [ |dens[r] - lval[t1]| + |lval[r] - dens[t2]| ]           sm += w_r
__global__ __launch_bounds__(256) void def_density_fwd_kernel(const float* __restrict__ pvec, const float* __restrict__ dens,
                                                              const float* __restrict__ lvec, const float* __restrict__ lval,
                                                              const float* __restrict__ mask, const int64_t* __restrict__ index1,
                                                              const int64_t* __restrict__ index2, int B, int N, int nc,
                                                              int defpart, double* __restrict__ part) {
    __shared__ double sh[12];
    double a = 0.0, e = 0.0, sm = 0.0;
    const int P = B * N;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < P; r += gridDim.x * blockDim.x) {
        const int b = r / N, i = r - b * N;
        const float w = def_weight(mask[(size_t)b * 3 * N + i], defpart);
        const int64_t i1 = index1[r], i2 = index2[r];
        float ce = 0.f, ae = 0.f;
        if (def_valid(i1, N)) {
            const size_t t1 = (size_t)b * N + i1;
            float s = 0.f;
            for (int c = 0; c < nc; ++c) s += lvec[t1 * nc + c] * logf(pvec[(size_t)r * nc + c] + 1e-10f);
            ce += s;
            ae += fabsf(dens[r] - lval[t1]);
        }
        if (def_valid(i2, N)) {
            const size_t t2 = (size_t)b * N + i2;
            float s = 0.f;
            for (int c = 0; c < nc; ++c) s += pvec[t2 * nc + c] * logf(lvec[(size_t)r * nc + c] + 1e-10f);
            ce += s;
            ae += fabsf(lval[r] - dens[t2]);
        }
        a += (double)ce * w; e += (double)ae * w; sm += w;
    }
    def_block_sum3(a, e, sm, sh);
    if (threadIdx.x == 0) { part[blockIdx.x * 3] = a; part[blockIdx.x * 3 + 1] = e; part[blockIdx.x * 3 + 2] = sm; }
}

// out = {kl + kl1, mae + mae1, sum w}:  -Dw a / sm,  Dw 0.05 e / sm   (lambda_2 = 1, lambda_1 = 0.05: :431-432)
__global__ __launch_bounds__(64) void def_density_finalize_kernel(const double* __restrict__ part, int nparts, float dweight,
                                                                  float* __restrict__ out) {
    double a = 0, e = 0, sm = 0;
    for (int i = threadIdx.x; i < nparts; i += 64) { a += part[i * 3]; e += part[i * 3 + 1]; sm += part[i * 3 + 2]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); e += __shfl_xor(e, o, 64); sm += __shfl_xor(sm, o, 64); }
    if (threadIdx.x == 0) {
        out[0] = (float)(-(double)dweight * a / sm);
        out[1] = (float)((double)dweight * 0.05 * e / sm);
        out[2] = (float)sm;
    }
}

// dpvec[b,i,c] = ck [ w_i lvec[idx1(i)][c] / (pvec[i][c] + 1e-10) + sum_{j: idx2(j) = i} w_j log(lvec[j][c] + 1e-10) ]
// ddens[b,i]   = cm [ w_i sign(dens_i - lval[idx1(i)]) - sum_{j: idx2(j) = i} w_j sign(lval_j - dens_i) ]
// ck = -g_kl Dw / sm, cm = g_mae Dw 0.05 / sm.  One workgroup per cloud.
__global__ __launch_bounds__(1024) void def_density_bwd_kernel(const float* __restrict__ pvec, const float* __restrict__ dens,
                                                               const float* __restrict__ lvec, const float* __restrict__ lval,
                                                               const float* __restrict__ mask, const int64_t* __restrict__ index1,
                                                               const int64_t* __restrict__ index2, int N, int NP, int nc, int defpart,
                                                               float dweight, const float* __restrict__ fwd_out,
                                                               const float* __restrict__ gkl, const float* __restrict__ gmae,
                                                               float* __restrict__ dp, float* __restrict__ dd) {
    extern __shared__ int gsm[];
    int* keys = gsm;
    int* seg = gsm + NP;
    const int b = blockIdx.x;
    def_group(index2 + (size_t)b * N, N, NP, keys, seg);
    const float* mb = mask + (size_t)b * 3 * N;
    const size_t base = (size_t)b * N;
    const float sm = fwd_out[2];
    const float ck = gkl ? -gkl[0] * dweight / sm : 0.f;
    const float cm = gmae ? gmae[0] * dweight * 0.05f / sm : 0.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const int q0 = seg[i], q1 = seg[i + 1];
        if (q1 - q0 > DEF_SHORT) continue;                      // a wave takes it below
        const size_t r = base + i;
        const int64_t i1 = index1[r];
        const bool v1 = def_valid(i1, N);
        const float wi = def_weight(mb[i], defpart);
        for (int c = 0; c < nc; ++c) {
            float g = v1 ? wi * lvec[(base + i1) * nc + c] / (pvec[r * nc + c] + 1e-10f) : 0.f;
            for (int q = q0; q < q1; ++q) {
                const int j = keys[q] & (NP - 1);
                g += def_weight(mb[j], defpart) * logf(lvec[(base + j) * nc + c] + 1e-10f);
            }
            dp[r * nc + c] = ck * g;
        }
        const float di = dens[r];
        float h = 0.f;
        if (v1) {
            const float df = di - lval[base + i1];
            h = wi * (float)((df > 0.f) - (df < 0.f));
        }
        for (int q = q0; q < q1; ++q) {
            const int j = keys[q] & (NP - 1);
            const float df = lval[base + j] - di;
            h -= def_weight(mb[j], defpart) * (float)((df > 0.f) - (df < 0.f));
        }
        dd[r] = cm * h;
    }
    for (int r0 = wave * 64; r0 < N; r0 += nw * 64) {
        const int ri = r0 + lane;
        unsigned long long todo = __ballot(ri < N && seg[ri + 1] - seg[ri] > DEF_SHORT);
        while (todo) {
            const int i = r0 + __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int q0 = seg[i], q1 = seg[i + 1];
            const size_t r = base + i;
            const int64_t i1 = index1[r];
            const bool v1 = def_valid(i1, N);
            const float wi = def_weight(mb[i], defpart);
            for (int c = 0; c < nc; ++c) {
                float g = 0.f;
                for (int q = q0 + lane; q < q1; q += 64) {
                    const int j = keys[q] & (NP - 1);
                    g += def_weight(mb[j], defpart) * logf(lvec[(base + j) * nc + c] + 1e-10f);
                }
                g = def_wave_sum(g);
                if (lane == 0) {
                    const float d = v1 ? wi * lvec[(base + i1) * nc + c] / (pvec[r * nc + c] + 1e-10f) : 0.f;
                    dp[r * nc + c] = ck * (d + g);
                }
            }
            const float di = dens[r];
            float h = 0.f;
            for (int q = q0 + lane; q < q1; q += 64) {
                const int j = keys[q] & (NP - 1);
                const float df = lval[base + j] - di;
                h -= def_weight(mb[j], defpart) * (float)((df > 0.f) - (df < 0.f));
            }
            h = def_wave_sum(h);
            if (lane == 0) {
                float d = 0.f;
                if (v1) {
                    const float df = di - lval[base + i1];
                    d = wi * (float)((df > 0.f) - (df < 0.f));
                }
                dd[r] = cm * (d + h);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// out[b][j][:] = x[b][idx(b,j)][:], W 32-bit words per row (bits copied: also gathers int64 labels as 2 words)
__global__ __launch_bounds__(256) void def_gather_kernel(const uint32_t* __restrict__ x, const int64_t* __restrict__ index, int B, int N,
                                                         int W, uint32_t* __restrict__ out) {
    const size_t total = (size_t)B * N * W;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / W;
        const int w = (int)(e - r * W);
        const int b = (int)(r / N);
        const int64_t t = index[r];
        out[e] = def_valid(t, N) ? x[((size_t)b * N + t) * W + w] : 0u;
    }
}

// dx[b][i][:] = sum_{j: idx(b,j) = i} dout[b][j][:] in a fixed order.  One workgroup per cloud.
__global__ __launch_bounds__(1024) void def_gather_bwd_kernel(const float* __restrict__ dout, const int64_t* __restrict__ index, int N,
                                                              int NP, int C, float* __restrict__ dx) {
    extern __shared__ int gsm[];
    int* keys = gsm;
    int* seg = gsm + NP;
    const int b = blockIdx.x;
    def_group(index + (size_t)b * N, N, NP, keys, seg);
    const size_t base = (size_t)b * N;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int e = threadIdx.x; e < N * C; e += blockDim.x) {
        const int i = e / C, c = e - i * C;
        if (seg[i + 1] - seg[i] > DEF_SHORT) continue;          // a wave takes it below
        float s = 0.f;
        for (int q = seg[i]; q < seg[i + 1]; ++q) s += dout[(base + (keys[q] & (NP - 1))) * C + c];
        dx[(base + i) * C + c] = s;
    }
    for (int r0 = wave * 64; r0 < N; r0 += nw * 64) {
        const int ri = r0 + lane;
        unsigned long long todo = __ballot(ri < N && seg[ri + 1] - seg[ri] > DEF_SHORT);
        while (todo) {
            const int i = r0 + __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            for (int c = 0; c < C; ++c) {
                float s = 0.f;
                for (int q = seg[i] + lane; q < seg[i + 1]; q += 64) s += dout[(base + (keys[q] & (NP - 1))) * C + c];
                s = def_wave_sum(s);
                if (lane == 0) dx[(base + i) * C + c] = s;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
static inline bool def_n_ok(int N) { return N >= 1 && N <= DEF_MAX_N; }
static inline size_t def_group_lds(int N) { return ((size_t)def_pow2(N) + N + 1) * sizeof(int); }

int launch_def_nearest(hipStream_t st, const float* pred, const float* gold, const float* mask, int B, int N, int64_t* index1,
                       int64_t* index2) {
    if (!def_n_ok(N)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(def_nearest_kernel, dim3((N + 255) / 256, B, 2), dim3(256), (size_t)N * sizeof(f32x4), st, pred, gold, mask, N,
                       index1, index2);
    return mlsp_launch_status();
}
int launch_def_normal_fwd(hipStream_t st, const float* pred, const float* lab, const float* mask, const int64_t* index1,
                          const int64_t* index2, int B, int N, int defpart, float weight, double* part, float* out) {
    if (!def_n_ok(N)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(def_normal_fwd_kernel, dim3(B), dim3(256), 0, st, pred, lab, mask, index1, index2, N, defpart, part);
    hipLaunchKernelGGL(def_normal_finalize_kernel, dim3(1), dim3(64), 0, st, part, B, weight, out);
    return mlsp_launch_status();
}
int launch_def_normal_bwd(hipStream_t st, const float* pred, const float* lab, const float* mask, const int64_t* index1,
                          const int64_t* index2, int B, int N, int defpart, float weight, const float* fwd_out, const float* gout,
                          float* dpred) {
    if (!def_n_ok(N)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(def_normal_bwd_kernel, dim3(B), dim3(1024), def_group_lds(N), st, pred, lab, mask, index1, index2, B, N,
                       def_pow2(N), defpart, weight, fwd_out, gout, dpred);
    return mlsp_launch_status();
}
int launch_def_density_fwd(hipStream_t st, const float* pvec, const float* dens, const float* lvec, const float* lval,
                           const float* mask, const int64_t* index1, const int64_t* index2, int B, int N, int nc, int defpart,
                           float dweight, double* part, float* out) {
    if (!def_n_ok(N)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(def_density_fwd_kernel, dim3(DEF_PARTS), dim3(256), 0, st, pvec, dens, lvec, lval, mask, index1, index2, B, N,
                       nc, defpart, part);
    hipLaunchKernelGGL(def_density_finalize_kernel, dim3(1), dim3(64), 0, st, part, DEF_PARTS, dweight, out);
    return mlsp_launch_status();
}
int launch_def_density_bwd(hipStream_t st, const float* pvec, const float* dens, const float* lvec, const float* lval,
                           const float* mask, const int64_t* index1, const int64_t* index2, int B, int N, int nc, int defpart,
                           float dweight, const float* fwd_out, const float* gkl, const float* gmae, float* dp, float* dd) {
    if (!def_n_ok(N)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(def_density_bwd_kernel, dim3(B), dim3(1024), def_group_lds(N), st, pvec, dens, lvec, lval, mask, index1, index2,
                       N, def_pow2(N), nc, defpart, dweight, fwd_out, gkl, gmae, dp, dd);
    return mlsp_launch_status();
}
int launch_def_gather(hipStream_t st, const uint32_t* x, const int64_t* index, int B, int N, int W, uint32_t* out) {
    if (!def_n_ok(N)) return MLSP_ERR_UNSUPPORTED;
    const size_t total = (size_t)B * N * W;
    const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(def_gather_kernel, dim3(blocks), dim3(256), 0, st, x, index, B, N, W, out);
    return mlsp_launch_status();
}
int launch_def_gather_bwd(hipStream_t st, const float* dout, const int64_t* index, int B, int N, int C, float* dx) {
    if (!def_n_ok(N)) return MLSP_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(def_gather_bwd_kernel, dim3(B), dim3(1024), def_group_lds(N), st, dout, index, N, def_pow2(N), C, dx);
    return mlsp_launch_status();
}
