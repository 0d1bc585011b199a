// Which kernel one farthest-point-sampling call runs on, decided in ONE place (host only: no HIP header, no kernel), like knn_plan.h for
// the kNN searches.  launch_fps (sa.hip) follows it; mlsp_fps_plan (api.hip) reports it, so that a test can state which kernel each of
// its cloud sizes reaches (tests/sa_restatement.py FPS_PLAN).
#pragma once

#define FPS_T 1024                 // threads of fps_kernel's one workgroup per cloud
#define FPS_PPT 8                  // ... and the points each of them keeps: N <= FPS_T * FPS_PPT
#define FPS2_MIN_N 64              // fps_kernel2 (4 waves, the arg-max as one 64-bit key reduced by DPP) takes FPS2_MIN_N <= N <= FPS2_MAX_N
#define FPS2_MAX_N 2048

enum { FPS_PLAN_NONE = 0, FPS_PLAN_KERNEL = 1, FPS_PLAN_KERNEL2 = 2 };

static inline int fps_plan(int N) {
    if (N <= 0 || N > FPS_T * FPS_PPT) return FPS_PLAN_NONE;
    return N >= FPS2_MIN_N && N <= FPS2_MAX_N ? FPS_PLAN_KERNEL2 : FPS_PLAN_KERNEL;
}
