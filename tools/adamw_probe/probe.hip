// Does torch's ROCm build contract AdamW's decay `param -= lr * weight_decay * param` (ATen/native/cuda/fused_adam_utils.cuh, ADAM_MODE::ADAMW:
// lr and weight_decay doubles, param a float) into a double fma?  One AdamW step under both lowerings (mode bit 1: contracted); the rest of
// the update is adam_one of csrc/optim.hip (its lowering settled by the Adam probe: profiles/r5_adam_lowering_probe.txt).
// tools/adamw_probe/run.py counts the elements that differ from torch._fused_adamw_.  Compiled with -ffp-contract=off: every fma below is
// written out, every other sum is rounded on its own.
#include <hip/hip_runtime.h>
#include <math.h>
extern "C" __global__ void probe(float* p, const float* g, float* m, float* v, int n, double lr, double b1, double b2, double wd, double eps,
                                 float bc1, float bc2s, int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float param = p[i], ea = m[i], es = v[i];
    const float grad = g[i];
    if (wd != 0.0) {
        if (mode & 1) param = (float)fma(-(lr * wd), (double)param, (double)param);
        else param = (float)((double)param - (lr * wd) * (double)param);
    }
    ea = (float)fma(b1, (double)ea, (1.0 - b1) * (double)grad);
    es = (float)fma(b2, (double)es, ((1.0 - b2) * (double)grad) * (double)grad);
    const float step_size = (float)(lr / (double)bc1);
    const float denom = (float)((double)(sqrtf(es) / bc2s) + eps);
    param -= step_size * ea / denom;
    p[i] = param; m[i] = ea; v[i] = es;
}
extern "C" int run_probe(float* p, const float* g, float* m, float* v, int n, double lr, double b1, double b2, double wd, double eps, int step,
                         int mode) {
    const float bc1 = (float)(1.0 - pow(b1, (double)(float)step));
    const float bc2s = (float)sqrt(1.0 - pow(b2, (double)(float)step));
    hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, p, g, m, v, n, lr, b1, b2, wd, eps, bc1, bc2s, mode);
    return (int)hipDeviceSynchronize();
}
