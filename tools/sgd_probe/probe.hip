// Which of the four `a + alpha * b` of torch's multi-tensor SGD does torch's ROCm build contract into an fma?  One SGD step under the 16
// lowerings (one bit per site); tools/sgd_probe/run.py counts the elements that differ from torch.optim.sgd.sgd(..., foreach=True).
// Compiled with -ffp-contract=off: every fma below is written out, every other sum is rounded on its own.
#include <hip/hip_runtime.h>
extern "C" __global__ void probe(float* p, const float* g, float* buf, int n, float wd, float mom, float damp1, float neg_lr, int nesterov,
                                 int maximize, int first, int mode) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float param = p[i], d = g[i];
    if (maximize) d = -d;
    if (wd != 0.f) d = (mode & 1) ? fmaf(wd, param, d) : d + wd * param;                     // _foreach_add(grads, params, alpha=wd)
    if (mom != 0.f) {
        float b = buf[i];
        if (first) b = d;                                                                      // clone of the gradient
        else {
            b = b * mom;                                                                       // _foreach_mul_(bufs, momentum)
            b = (mode & 2) ? fmaf(damp1, d, b) : b + damp1 * d;                                // _foreach_add_(bufs, grads, alpha=1 - dampening)
        }
        buf[i] = b;
        d = nesterov ? ((mode & 4) ? fmaf(mom, b, d) : d + mom * b) : b;                      // _foreach_add_(grads, bufs, alpha=momentum)
    }
    p[i] = (mode & 8) ? fmaf(neg_lr, d, param) : param + neg_lr * d;                           // _foreach_add_(params, grads, alpha=-lr)
}
extern "C" int run_probe(float* p, const float* g, float* buf, int n, double lr, double momentum, double dampening, double wd, int nesterov,
                         int maximize, int first, int mode) {
    // every scalar reaches the foreach op as a Python float and becomes a float alpha there; 1 - dampening and -lr are formed in double
    hipLaunchKernelGGL(probe, dim3((n + 255) / 256), dim3(256), 0, 0, p, g, buf, n, (float)wd, (float)momentum, (float)(1.0 - dampening),
                       (float)(-lr), nesterov, maximize, first, mode);
    return (int)hipDeviceSynchronize();
}
