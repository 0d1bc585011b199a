// Input corruption of the source/target branches: voxel-region assignment (utils/pc_utils.py:33-73) and
// the "volume_based_voxels" deformation of MLSP/mlsp.py:10-51 -- in the reference a Python loop over the batch x 27 regions
// with host round trips (1.16 s per batch on the CPU).  One kernel each; the random inputs (region visiting order, Gaussian
// noise) are ARGUMENTS, so the result is a pure function that tests can compare with the reference's own arithmetic.
#include "common.h"

// Y[b][j] = id of the voxel (x*n*n + y*n + z) whose OPEN box contains the clamped point, 0 when none does (points on a
// voxel face, points with a NaN coordinate): the reference labels by overwriting inside three nested loops, which is the same thing because the boxes
// are disjoint.  thr[0..n] are the fp32 box edges -1 + i*d exactly as torch rounds the Python scalars; clip = fp32(0.99999999).
__global__ __launch_bounds__(256) void region_assign_kernel(const float* __restrict__ X, int C, int N, int total, const float* __restrict__ thr,
                                                            int n, float clip, int* __restrict__ Y) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int b = t / N, j = t % N;
    const float* xb = X + (size_t)b * C * N;
    int id[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float v = xb[(size_t)a * N + j];
        v = fminf(fmaxf(v, -clip), clip);      // a NaN becomes -clip; fp32(0.99999999) is 1, the outer face thr[0]: no box, like the reference's NaN
        int r = -1;
        for (int i = 0; i < n; ++i)
            if (thr[i] < v && v < thr[i + 1]) r = i;
        id[a] = r;
    }
    Y[t] = (id[0] < 0 || id[1] < 0 || id[2] < 0) ? 0 : (id[0] * n + id[1]) * n + id[2];
}

// One workgroup per cloud: histogram of the region ids, then the first `groups` regions of the visiting order that hold
// >= min_pts points are collapsed: X[b][0:3][j] = centre + noise[b][0:3][j] (noise already scaled), mask[b][0:3][j] = 1.
__global__ __launch_bounds__(256) void deform_regions_kernel(float* __restrict__ X, int C, int N, const int* __restrict__ regions,
                                                             const int* __restrict__ order, int nreg, const float* __restrict__ lookup,
                                                             const float* __restrict__ noise, int min_pts, int groups,
                                                             float* __restrict__ mask) {
    __shared__ int hist[512];
    __shared__ int chosen[512];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int r = tid; r < nreg; r += 256) { hist[r] = 0; chosen[r] = 0; }
    __syncthreads();
    const int* rb = regions + (size_t)b * N;
    for (int j = tid; j < N; j += 256) atomicAdd(&hist[rb[j]], 1);
    __syncthreads();
    if (tid == 0) {
        int it = 0;
        for (int q = 0; q < nreg && it < groups; ++q) {
            const int r = order[q];
            if (hist[r] >= min_pts) { chosen[r] = 1; ++it; }
        }
    }
    __syncthreads();
    float* xb = X + (size_t)b * C * N;
    float* mb = mask + (size_t)b * C * N;
    const float* nb = noise + (size_t)b * 3 * N;
    for (int j = tid; j < N; j += 256) {
        const int r = rb[j];
        const bool hit = chosen[r] != 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (hit) xb[(size_t)a * N + j] = lookup[r * 3 + a] + nb[(size_t)a * N + j];
            mb[(size_t)a * N + j] = hit ? 1.f : 0.f;
        }
        for (int a = 3; a < C; ++a) mb[(size_t)a * N + j] = 0.f;
    }
}

// scan_input / p_scan (MLSP/mlsp.py:54-89): every cloud is rotated by its own random matrix R (host float64, as the reference),
// projected on a pixel grid along +x, and per occupied cell only the point with the largest rotated x survives ("visible"
// from that side; ties -> lowest index, like the reference's sequential scan).  X [B][N][C] point-major (as the trainer holds it
// here); Xs gets the survivors (all other points zero), mask is 1 everywhere except the first three channels of the survivors.
// float64 like numpy: rot = ((p0*R0c + p1*R1c) + p2*R2c), cell = trunc(((z+1)/2*pixel)*pixel + ((y+1)/2)*pixel).
__global__ __launch_bounds__(1024) void scan_select_kernel(const float* __restrict__ X, int N, int C, const double* __restrict__ R, int pixel,
                                                           float* __restrict__ Xs, float* __restrict__ mask) {
    extern __shared__ double ssm[];
    double* xr = ssm;                      // [N] rotated x
    int* cell = (int*)(ssm + N);           // [N]
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* xb = X + (size_t)b * N * C;
    const double* Rb = R + (size_t)b * 9;
    for (int j = tid; j < N; j += 1024) {
        const double p0 = xb[(size_t)j * C], p1 = xb[(size_t)j * C + 1], p2 = xb[(size_t)j * C + 2];
        const double rx = (p0 * Rb[0] + p1 * Rb[3]) + p2 * Rb[6];
        const double ry = (p0 * Rb[1] + p1 * Rb[4]) + p2 * Rb[7];
        const double rz = (p0 * Rb[2] + p1 * Rb[5]) + p2 * Rb[8];
        xr[j] = rx;
        cell[j] = (int)(((rz + 1.0) / 2.0 * pixel) * pixel + (ry + 1.0) / 2.0 * pixel);
    }
    __syncthreads();
    for (int j = tid; j < N; j += 1024) {
        const int cj = cell[j];
        const double xj = xr[j];
        bool win = true;
        for (int i = 0; i < N; ++i) {
            const bool same = cell[i] == cj;
            win = win && !(same && (xr[i] > xj || (xr[i] == xj && i < j)));
        }
        for (int c = 0; c < C; ++c) {
            const size_t o = ((size_t)b * N + j) * C + c;
            Xs[o] = win ? xb[(size_t)j * C + c] : 0.f;
            mask[o] = (win && c < 3) ? 0.f : 1.f;
        }
    }
}

// deform_input(..., 'volume_based_radius') = pc_utils.collapse_to_point (utils/pc_utils.py:76-111), one workgroup per cloud:
//   pd[i][j] = (xx_j + (-2 x_i.x_j)) + xx_i          (fp32, the reference's association; dot as an fmaf chain over the 3 coordinates)
//   a point is a candidate when >= min_pts points lie within the radius (pd <= r2, itself included); one candidate is picked
//   (uniformly by `u` in [0,1), or the given index `choice`), and every point within the radius of it is replaced by
//   centre + noise (noise pre-scaled), mask = 1 on its three coordinates.  No candidate: the cloud is left untouched (the
//   reference raises).  X [B][3][N]; chosen_out[b] = the picked point or -1.
__global__ __launch_bounds__(1024) void collapse_to_point_kernel(float* __restrict__ X, int N, const int* __restrict__ choice,
                                                                 const float* __restrict__ u, const float* __restrict__ noise, float r2,
                                                                 int min_pts, float* __restrict__ mask, int* __restrict__ chosen_out) {
    extern __shared__ float csm[];
    float* px = csm; float* py = px + N; float* pz = py + N; float* xx = pz + N;      // [N] each
    int* cand = (int*)(xx + N);                                                           // [N] candidate flags
    __shared__ int s_ncand, s_pick;
    const int b = blockIdx.x, tid = threadIdx.x;
    float* xb = X + (size_t)b * 3 * N;
    for (int j = tid; j < N; j += 1024) {
        const float a = xb[j], c = xb[N + j], d = xb[2 * N + j];
        px[j] = a; py[j] = c; pz[j] = d;
        xx[j] = (a * a + c * c) + d * d;
    }
    if (tid == 0) { s_ncand = 0; s_pick = -1; }
    __syncthreads();
    int my = 0;
    for (int i = tid; i < N; i += 1024) {
        const float a = px[i], c = py[i], d = pz[i], xi = xx[i];
        int cnt = 0;
        for (int j = 0; j < N; ++j) {
            const float dot = fmaf(d, pz[j], fmaf(c, py[j], a * px[j]));
            const float pd = (xx[j] + (-2.f * dot)) + xi;
            cnt += pd <= r2;
        }
        const int f = cnt >= min_pts;
        cand[i] = f; my += f;
    }
    atomicAdd(&s_ncand, my);
    __syncthreads();
    const int ncand = s_ncand;
    if (ncand > 0) {
        int want = (choice && choice[b] >= 0) ? -2 : (int)(u[b] * (float)ncand);
        if (want >= ncand) want = ncand - 1;
        if (want == -2) { if (tid == 0) s_pick = choice[b]; }
        else {
            for (int i = tid; i < N; i += 1024) {
                if (!cand[i]) continue;
                int rank = 0;
                for (int j = 0; j < i; ++j) rank += cand[j];
                if (rank == want) s_pick = i;
            }
        }
    }
    __syncthreads();
    const int p = s_pick;
    if (tid == 0) chosen_out[b] = p;
    float* mb = mask + (size_t)b * 3 * N;
    const float* nb = noise + (size_t)b * 3 * N;
    float ca = 0.f, cc = 0.f, cd = 0.f, xp = 0.f;
    if (p >= 0) { ca = px[p]; cc = py[p]; cd = pz[p]; xp = xx[p]; }
    for (int j = tid; j < N; j += 1024) {
        bool hit = false;
        if (p >= 0) {
            const float dot = fmaf(cd, pz[j], fmaf(cc, py[j], ca * px[j]));
            hit = ((xx[j] + (-2.f * dot)) + xp) <= r2;
        }
        if (hit) { xb[j] = ca + nb[j]; xb[N + j] = cc + nb[N + j]; xb[2 * N + j] = cd + nb[2 * N + j]; }
        const float m = hit ? 1.f : 0.f;
        mb[j] = m; mb[N + j] = m; mb[2 * N + j] = m;
    }
}

int launch_collapse_to_point(hipStream_t st, float* X, int B, int N, const int* choice, const float* u, const float* noise, float r2,
                             int min_pts, float* mask, int* chosen) {
    if (!X || !noise || !mask || !chosen || (!u && !choice) || B <= 0 || N <= 0 || min_pts <= 0) return MLSP_ERR_ARG;
    const size_t lds = (size_t)N * 5 * sizeof(float);
    if (lds > 150 * 1024) return MLSP_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        hipError_t e = mlsp_lds_limit((const void*)collapse_to_point_kernel, lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(collapse_to_point_kernel, dim3(B), dim3(1024), lds, st, X, N, choice, u, noise, r2, min_pts, mask, chosen);
    return mlsp_launch_status();
}

int launch_scan_select(hipStream_t st, const float* X, int B, int N, int C, const double* R, int pixel, float* Xs, float* mask) {
    if (!X || !R || !Xs || !mask || B <= 0 || N <= 0 || C < 3 || pixel <= 0) return MLSP_ERR_ARG;
    const size_t lds = (size_t)N * (sizeof(double) + sizeof(int));
    if (lds > 150 * 1024) return MLSP_ERR_UNSUPPORTED;
    if (lds > 64 * 1024) {
        hipError_t e = mlsp_lds_limit((const void*)scan_select_kernel, lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(scan_select_kernel, dim3(B), dim3(1024), lds, st, X, N, C, R, pixel, Xs, mask);
    return mlsp_launch_status();
}

int launch_region_assign(hipStream_t st, const float* X, int B, int C, int N, const float* thr, int n, float clip, int* Y) {
    if (!X || !thr || !Y || B <= 0 || C < 3 || N <= 0 || n <= 0 || n > 8) return MLSP_ERR_ARG;
    const int total = B * N;
    hipLaunchKernelGGL(region_assign_kernel, dim3((total + 255) / 256), dim3(256), 0, st, X, C, N, total, thr, n, clip, Y);
    return mlsp_launch_status();
}

int launch_deform_regions(hipStream_t st, float* X, int B, int C, int N, const int* regions, const int* order, int nreg, const float* lookup,
                          const float* noise, int min_pts, int groups, float* mask) {
    if (!X || !regions || !order || !lookup || !noise || !mask || B <= 0 || C < 3 || N <= 0 || nreg <= 0 || nreg > 512 || groups <= 0)
        return MLSP_ERR_ARG;
    hipLaunchKernelGGL(deform_regions_kernel, dim3(B), dim3(256), 0, st, X, C, N, regions, order, nreg, lookup, noise, min_pts, groups, mask);
    return mlsp_launch_status();
}

// Input transform of DGCNN (PointDA/Models.py:113, x = matmul(T, x)): out[p][i] = sum_j T[b][i][j] * x[p][j] on point-major
// [P][3] rows, T [B][3][3].  A 3x3 batched matmul through the vendor GEMM is three launches of transposes and tiles; here one
// streaming pass each way.  Backward: dx[p][j] = sum_i dout[p][i] T[b][i][j];  dT[b][i][j] = sum_p dout[p][i] x[p][j] (one workgroup
// per cloud, fixed reduction order).
__global__ __launch_bounds__(256) void transform3_fwd_kernel(const float* __restrict__ x, const float* __restrict__ T, int N, int P,
                                                             float* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float* t = T + (size_t)(p / N) * 9;
    const float a = x[(size_t)p * 3], b = x[(size_t)p * 3 + 1], c = x[(size_t)p * 3 + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) out[(size_t)p * 3 + i] = fmaf(t[3 * i + 2], c, fmaf(t[3 * i + 1], b, t[3 * i] * a));
}
__global__ __launch_bounds__(256) void transform3_bwd_kernel(const float* __restrict__ x, const float* __restrict__ T,
                                                             const float* __restrict__ dout, int N, float* __restrict__ dx,
                                                             float* __restrict__ dT) {
    __shared__ float red[4][9];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* t = T + (size_t)b * 9;
    float acc[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) acc[e] = 0.f;
    for (int n = tid; n < N; n += 256) {
        const size_t p = (size_t)b * N + n;
        const float g0 = dout[p * 3], g1 = dout[p * 3 + 1], g2 = dout[p * 3 + 2];
        const float x0 = x[p * 3], x1 = x[p * 3 + 1], x2 = x[p * 3 + 2];
        if (dx) {
#pragma unroll
            for (int j = 0; j < 3; ++j) dx[p * 3 + j] = fmaf(g2, t[6 + j], fmaf(g1, t[3 + j], g0 * t[j]));
        }
        acc[0] = fmaf(g0, x0, acc[0]); acc[1] = fmaf(g0, x1, acc[1]); acc[2] = fmaf(g0, x2, acc[2]);
        acc[3] = fmaf(g1, x0, acc[3]); acc[4] = fmaf(g1, x1, acc[4]); acc[5] = fmaf(g1, x2, acc[5]);
        acc[6] = fmaf(g2, x0, acc[6]); acc[7] = fmaf(g2, x1, acc[7]); acc[8] = fmaf(g2, x2, acc[8]);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) {
        float v = acc[e];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[w][e] = v;
    }
    __syncthreads();
    if (tid < 9) dT[(size_t)b * 9 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}
int launch_transform3_fwd(hipStream_t st, const float* x, const float* T, int B, int N, float* out) {
    if (!x || !T || !out || B <= 0 || N <= 0) return MLSP_ERR_ARG;
    const int P = B * N;
    hipLaunchKernelGGL(transform3_fwd_kernel, dim3((P + 255) / 256), dim3(256), 0, st, x, T, N, P, out);
    return mlsp_launch_status();
}
int launch_transform3_bwd(hipStream_t st, const float* x, const float* T, const float* dout, int B, int N, float* dx, float* dT) {
    if (!x || !T || !dout || !dT || B <= 0 || N <= 0) return MLSP_ERR_ARG;
    hipLaunchKernelGGL(transform3_bwd_kernel, dim3(B), dim3(256), 0, st, x, T, dout, N, dx, dT);
    return mlsp_launch_status();
}
