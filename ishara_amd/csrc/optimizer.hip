// Fused multi-tensor optimizer over the flat fp32 parameter buffer:
// tfa.optimizers.RectifiedAdam(sma_threshold=4) wrapped in tfa.optimizers.Lookahead(
// sync_period=5, slow_step_size=0.5) — conv-hybrid-model.ipynb c7:68-69.  The step-dependent
// scalars (bias corrections, rectification r_t, sync flag) are computed on the host.
#include "kernels.h"

// the update of element i with gradient g: shared by the two kernels below
__device__ __forceinline__ void radam_lookahead_update(int64_t i, float g, float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ slow, const RAdamArgs& a) {
    const float mi = a.beta1 * m[i] + (1.f - a.beta1) * g;
    const float vi = a.beta2 * v[i] + (1.f - a.beta2) * g * g;
    m[i] = mi; v[i] = vi;
    const float mh = mi * a.c1;
    float upd = a.rect ? a.r_t * mh / (sqrtf(vi * a.c2) + a.eps) : mh;
    float th = theta[i];
    if (a.wd != 0.f) upd += a.wd * th;
    th -= a.lr * upd;
    if (a.sync) {
        const float sl = slow[i] + a.slow_step * (th - slow[i]);
        slow[i] = sl;
        th = sl;
    }
    theta[i] = th;
}

__global__ __launch_bounds__(256) void radam_lookahead_kernel(float* __restrict__ theta, const float* __restrict__ grad,
                                                              float* __restrict__ m, float* __restrict__ v, float* __restrict__ slow,
                                                              int64_t n, RAdamArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) radam_lookahead_update(i, grad[i], theta, m, v, slow, a);
}

// The same update behind the device record of grad_stats (grad_ops.hip): the gradient is scaled by st->coef, and with `skip` a step whose
// gradient holds a NaN or Inf writes nothing to theta / m / v / slow and counts itself in st->skipped.  No other arithmetic differs.
__global__ __launch_bounds__(256) void radam_lookahead_ex_kernel(float* __restrict__ theta, const float* __restrict__ grad,
                                                                 float* __restrict__ m, float* __restrict__ v, float* __restrict__ slow,
                                                                 int64_t n, RAdamArgs a, ishara_grad_stats* st, int skip) {
    const int nonfinite = st->nonfinite;      // read once per thread, before the loop
    const float coef = st->coef;
    if (skip && nonfinite > 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) st->skipped += 1;
        return;
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) radam_lookahead_update(i, grad[i] * coef, theta, m, v, slow, a);
}

int launch_radam_lookahead(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n,
                           RAdamArgs a, hipStream_t s) {
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(radam_lookahead_kernel, dim3(grid), dim3(256), 0, s, theta, grad, m, v, slow, n, a);
    return launch_rc();
}

int launch_radam_lookahead_ex(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n,
                              RAdamArgs a, ishara_grad_stats* st, int skip, hipStream_t s) {
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(radam_lookahead_ex_kernel, dim3(grid), dim3(256), 0, s, theta, grad, m, v, slow, n, a, st, skip);
    return launch_rc();
}

__global__ void scale_kernel(float* __restrict__ x, int64_t n, float scale) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] *= scale;
}
int launch_scale(float* x, int64_t n, float scale, hipStream_t s) {
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(scale_kernel, dim3(grid), dim3(256), 0, s, x, n, scale);
    return launch_rc();
}
