// The bodies of batchprep_kernel (batchprep.hip), one function per phase between two workgroup barriers, each a function of (thread) or of
// one point: batchprep.hip calls them with threadIdx and a __syncthreads() between phases, tools/batchprep_host_check runs them on the
// host, one call per thread and phase, against exact-size heap buffers.  No lane talks to another inside a phase; the one exception, the
// DPP arg-max of the sampling loop, is device-only and the host walk takes a plain maximum over the same keys.
//
// One workgroup prepares one cloud of n <= BP_MAXN points (PointDA/data/dataloader.py __getitem__):
//   unit cube  c = sum x / n and r = max sqrt(|x - c|^2) in double, u = f32((x - c) / r): one rounding of the exact quotient's double
//   pre-rotate v = f32((u0 R[0][k] + u1 R[1][k]) + u2 R[2][k]) in double (numpy: a float32 array times a float64 matrix, then astype)
//   sampling   farthest point sampling on v in fp32, d = (dx dx + dy dy) + dz dz, running minimum from 1e10, first index wins
//   post-rotate the same product with Q on the chosen points;  jitter  f32(f64(w) + clip(sigma noise)) (numpy's in-place float32 += float64)
// The prologue's sums run over BP_LANES = 256 virtual lanes whatever the workgroup's width, so a cloud's bits do not depend on the batch
// it travels in: lane l adds the points l, l + 256, ... in ascending order, 64 group leaders add four lanes each, every thread adds the
// 64 groups in ascending order.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "rowtile.h"

#define BP_MAXN 8192
#define BP_PPT 8                                           // points per thread: 256 threads up to 2048 points, 1024 beyond
#define BP_LANES 256
#define BP_GROUPS 64
#define BP_CHUNK 512                                       // clouds per launch (their counts and flags travel as kernel arguments)
#define BP_F_PRE 1                                         // flag bits of a cloud
#define BP_F_POST 2
#define BP_F_JITTER 4
#define BP_F_RAW 8                                         // no unit-cube scaling: the coordinates pass through
#define BP_F_ALL 15

// byte offsets into the workgroup's LDS block for clouds of at most ncap points, S samples, nw waves
struct BpLds { unsigned cx, part, partm, wsum, wmax, slot, sel, bytes; };
RT_HD BpLds bp_lds(int ncap, int S, int nw) {
    BpLds l;
    l.cx = 0;                                              // [ncap][3] floats
    l.part = (unsigned)(((size_t)12 * ncap + 15) & ~(size_t)15);   // [256][3] doubles
    l.partm = l.part + BP_LANES * 3 * 8;                   // [256] doubles
    l.wsum = l.partm + BP_LANES * 8;                       // [64][3] doubles
    l.wmax = l.wsum + BP_GROUPS * 3 * 8;                   // [64] doubles
    l.slot = l.wmax + BP_GROUPS * 8;                       // [2][nw] keys
    l.sel = l.slot + 2 * nw * 8;                           // [S] ints
    l.bytes = l.sel + 4 * (unsigned)S;
    return l;
}

// ---- prologue ------------------------------------------------------------------------------------------------------------------------
RT_HD void bp_stage(const float* xb, int ld, int j, float* cx) {
    cx[3 * j] = xb[(size_t)j * ld]; cx[3 * j + 1] = xb[(size_t)j * ld + 1]; cx[3 * j + 2] = xb[(size_t)j * ld + 2];
}
// lane < BP_LANES
RT_HD void bp_sum_lane(const float* cx, int n, int lane, double* part) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll 2
    for (int j = lane; j < n; j += BP_LANES) { s0 += (double)cx[3 * j]; s1 += (double)cx[3 * j + 1]; s2 += (double)cx[3 * j + 2]; }
    part[3 * lane] = s0; part[3 * lane + 1] = s1; part[3 * lane + 2] = s2;
}
// g < BP_GROUPS
RT_HD void bp_sum_group(const double* part, int g, double* wsum) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double s = part[3 * (4 * g) + k];
        for (int q = 1; q < 4; ++q) s += part[3 * (4 * g + q) + k];
        wsum[3 * g + k] = s;
    }
}
// every thread
RT_HD void bp_centroid(const double* wsum, int n, double c[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double s = wsum[k];
#pragma unroll 4
        for (int g = 1; g < BP_GROUPS; ++g) s += wsum[3 * g + k];
        c[k] = s / (double)n;
    }
}
RT_HD double bp_dist2(const float* p, const double c[3]) {
    const double dx = (double)p[0] - c[0], dy = (double)p[1] - c[1], dz = (double)p[2] - c[2];
    return (dx * dx + dy * dy) + dz * dz;
}
// lane < BP_LANES.  A NaN distance never replaces the maximum (the comparison is false)
RT_HD void bp_max_lane(const float* cx, int n, int lane, const double c[3], double* partm) {
    double m = 0.0;
#pragma unroll 2
    for (int j = lane; j < n; j += BP_LANES) { const double d = bp_dist2(cx + 3 * j, c); m = d > m ? d : m; }
    partm[lane] = m;
}
RT_HD void bp_max_group(const double* partm, int g, double* wmax) {
    double m = partm[4 * g];
    for (int q = 1; q < 4; ++q) m = partm[4 * g + q] > m ? partm[4 * g + q] : m;
    wmax[g] = m;
}
// every thread: max sqrt(d2) = sqrt(max d2), sqrt is monotone
RT_HD double bp_radius(const double* wmax) {
    double m = wmax[0];
#pragma unroll 4
    for (int g = 1; g < BP_GROUPS; ++g) m = wmax[g] > m ? wmax[g] : m;
    return sqrt(m);
}
// v = f32((u0 R[0][k] + u1 R[1][k]) + u2 R[2][k]), R row-major
RT_HD void bp_rotate(const float u[3], const double* R, float v[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (float)(((double)u[0] * R[k] + (double)u[1] * R[3 + k]) + (double)u[2] * R[6 + k]);
}
// point j of the cloud, in place in cx
RT_HD void bp_norm_rotate(float* cx, int j, int fl, const double c[3], double r, const double* R) {
    float p[3], u[3] = {cx[3 * j], cx[3 * j + 1], cx[3 * j + 2]};
    if (!(fl & BP_F_RAW)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) u[k] = (float)(((double)u[k] - c[k]) / r);
    }
    if (fl & BP_F_PRE) bp_rotate(u, R, p);
    else { p[0] = u[0]; p[1] = u[1]; p[2] = u[2]; }
    cx[3 * j] = p[0]; cx[3 * j + 1] = p[1]; cx[3 * j + 2] = p[2];
}

// ---- sampling ------------------------------------------------------------------------------------------------------------------------
// one point's part of one step: the running minimum moves, the key orders by (distance, lower index).  Distances are >= 0, so their bit
// patterns order like the floats; a NaN distance leaves the minimum where it is (fminf returns its other argument).  A register slot past
// the end of the cloud starts with the minimum 0 and coordinates 0: it stays 0, and its key loses to every real point's.
RT_HD unsigned long long bp_fps_point(float px, float py, float pz, float& dmin, float fx, float fy, float fz, int j) {
    const float dx = px - fx, dy = py - fy, dz = pz - fz;
    const float d = (dx * dx + dy * dy) + dz * dz;
    dmin = fminf(dmin, d);
    return ((unsigned long long)__builtin_bit_cast(unsigned, dmin) << 32) | (unsigned)(~j);
}
RT_HD int bp_key_index(unsigned long long key) { return (int)(~(unsigned)key); }
RT_HD int bp_clamp_start(int s, int n) { return s < 0 ? 0 : s >= n ? n - 1 : s; }

// ---- epilogue ------------------------------------------------------------------------------------------------------------------------
// sample i of the cloud: the point `src` of cx -> out[3], through the post-rotation and the jitter the flags ask for
RT_HD void bp_epilogue(const float* cx, int src, int fl, const double* Q, const double* nz, double sigma, double clip, float* out) {
    const float p[3] = {cx[3 * src], cx[3 * src + 1], cx[3 * src + 2]};
    float w[3] = {p[0], p[1], p[2]};
    if (fl & BP_F_POST) bp_rotate(p, Q, w);
    if (fl & BP_F_JITTER) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            double t = sigma * nz[k];
            t = t < -clip ? -clip : t;
            t = t > clip ? clip : t;
            w[k] = (float)((double)w[k] + t);
        }
    }
    out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
}
