// Fused multi-tensor optimizer over the flat fp32 parameter buffer:
// tfa.optimizers.RectifiedAdam(sma_threshold=4) wrapped in tfa.optimizers.Lookahead(
// sync_period=5, slow_step_size=0.5) — conv-hybrid-model.ipynb c7:68-69.  The step-dependent
// scalars (bias corrections, rectification r_t, sync flag) are computed on the host.
#include <cmath>

#include "seg_chunks.h"

// the update of element i with gradient g: shared by every kernel below.  hipcc contracts a * b + c into an FMA where it pleases, and what
// it pleases depends on the code around the call (the four lanes of a float4 fused b2 * v + ((1 - b2) * g) * g the other way round), so
// the fusions are written out under the pragma: they are the ones the two plain kernels have always been compiled to (their ISA is
// unchanged by this), and every caller, scalar or vector, now gets the same bits.
__device__ __forceinline__ void radam_lookahead_update(int64_t i, float g, float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v,
                                                       float* __restrict__ slow, const RAdamArgs& a) {
#pragma clang fp contract(off)
    const float mi = a.beta1 * m[i] + (1.f - a.beta1) * g;                                   // two products, one sum: three roundings
    const float vi = __builtin_fmaf(g, (1.f - a.beta2) * g, a.beta2 * v[i]);
    m[i] = mi; v[i] = vi;
    const float mh = mi * a.c1;
    float upd = a.rect ? a.r_t * mh / (sqrtf(vi * a.c2) + a.eps) : mh;
    float th = theta[i];
    if (a.wd != 0.f) upd = __builtin_fmaf(a.wd, th, upd);
    th = __builtin_fmaf(-a.lr, upd, th);
    if (a.sync) {
        const float sl = __builtin_fmaf(a.slow_step, th - slow[i], slow[i]);
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

// the step-dependent scalars of step `iteration` (1-based), evaluated in fp64 on the host
RAdamArgs radam_args(int32_t iteration, float lr, float wd) {
    const double t = (double)iteration, b1 = 0.9, b2 = 0.999;
    const double b1p = pow(b1, t), b2p = pow(b2, t);
    const double sma_inf = 2.0 / (1.0 - b2) - 1.0;
    const double sma_t = sma_inf - 2.0 * t * b2p / (1.0 - b2p);
    RAdamArgs a;
    a.lr = lr; a.wd = wd; a.beta1 = (float)b1; a.beta2 = (float)b2; a.eps = 1e-7f;
    a.c1 = (float)(1.0 / (1.0 - b1p)); a.c2 = (float)(1.0 / (1.0 - b2p));
    a.rect = sma_t >= 4.0 ? 1 : 0;       // sma_threshold = 4 (c7:68)
    a.r_t = a.rect ? (float)sqrt(fmax((sma_t - 4.0) / (sma_inf - 4.0) * (sma_t - 2.0) / (sma_inf - 2.0) * sma_inf / sma_t, 0.0)) : 0.f;
    a.sync = (iteration % 5 == 0) ? 1 : 0;   // Lookahead(sync_period=5, slow_step_size=0.5) (c7:69)
    a.slow_step = 0.5f;
    return a;
}

// ---- parameter groups: the same update over a segment table, one row of options per segment ------------------------------------------
// The chunks of seg_chunks.h (AWP's): a workgroup takes chunk c, finds its segment by bisection, reads the segment's 16-byte row with
// wave-uniform loads and either leaves the chunk alone (frozen: no load, no store) or runs radam_lookahead_update over it with
// lr * lr_scale and wd * wd_scale.  theta, grad, m, v and slow share the element index and 16-byte aligned bases, so one head / body /
// tail cut serves the five: the body moves as float4s through registers, the function above working on the four lanes in place.
// HBM-bound: 28 bytes per unfrozen element (36 on a Lookahead sync step), nothing for a frozen one, plus the tables, which stay in L2.
__device__ __forceinline__ RAdamArgs group_args(RAdamArgs a, const ishara_param_group& r) {
    a.lr = a.lr * r.lr_scale;      // one fp32 multiply each; a product of 0 takes the a.wd != 0.f branch of the update as wd = 0 does
    a.wd = a.wd * r.wd_scale;
    return a;
}

template <bool REC>
__global__ __launch_bounds__(SEG_THREADS) void radam_lookahead_groups_kernel(float* __restrict__ theta, const float* __restrict__ grad, float* __restrict__ m,
                                                                             float* __restrict__ v, float* __restrict__ slow, int64_t n, int64_t bound, RAdamArgs a0,
                                                                             ishara_grad_stats* st, int skip, const int64_t* __restrict__ seg_off,
                                                                             const ishara_param_group* __restrict__ groups, int S, const int64_t* __restrict__ first) {
    float coef = 1.f;
    if (REC) {
        const int nonfinite = st->nonfinite;      // read once per thread, before the loop (as radam_lookahead_ex_kernel)
        coef = st->coef;
        if (skip && nonfinite > 0) {
            if (blockIdx.x == 0 && threadIdx.x == 0) st->skipped += 1;
            return;
        }
    }
    const int64_t chunks = first[S] < bound ? first[S] : bound;      // == first[S] for a table that keeps its contract
    float4* __restrict__ th4 = reinterpret_cast<float4*>(theta);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
    float4* __restrict__ sl4 = reinterpret_cast<float4*>(slow);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(grad);
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const AwpSpan p = awp_span(seg_off, first, S, n, c);
        const ishara_param_group row = groups[p.seg];
        if (row.frozen != 0) continue;
        const RAdamArgs a = group_args(a0, row);
        const int64_t h = p.e0 + threadIdx.x, t = p.a1 + threadIdx.x;
        if (h < p.a0) radam_lookahead_update(h, REC ? grad[h] * coef : grad[h], theta, m, v, slow, a);
        for (int64_t q = p.a0 / SEG_VEC + threadIdx.x; q < p.a1 / SEG_VEC; q += SEG_THREADS) {
            const float4 gq = g4[q], tq = th4[q], mq = m4[q], vq = v4[q];
            float g[SEG_VEC] = {gq.x, gq.y, gq.z, gq.w}, th[SEG_VEC] = {tq.x, tq.y, tq.z, tq.w};
            float mm[SEG_VEC] = {mq.x, mq.y, mq.z, mq.w}, vv[SEG_VEC] = {vq.x, vq.y, vq.z, vq.w}, sl[SEG_VEC] = {0.f, 0.f, 0.f, 0.f};
            if (a.sync) { const float4 sq = sl4[q]; sl[0] = sq.x; sl[1] = sq.y; sl[2] = sq.z; sl[3] = sq.w; }      // slow is touched on sync steps only
#pragma unroll
            for (int k = 0; k < SEG_VEC; ++k) radam_lookahead_update(k, REC ? g[k] * coef : g[k], th, mm, vv, sl, a);
            th4[q] = make_float4(th[0], th[1], th[2], th[3]);
            m4[q] = make_float4(mm[0], mm[1], mm[2], mm[3]);
            v4[q] = make_float4(vv[0], vv[1], vv[2], vv[3]);
            if (a.sync) sl4[q] = make_float4(sl[0], sl[1], sl[2], sl[3]);
        }
        if (t < p.e1) radam_lookahead_update(t, REC ? grad[t] * coef : grad[t], theta, m, v, slow, a);
    }
}

// g = +0.0f (the word 0) over the chunks of the frozen segments; no other word is read or written
__global__ __launch_bounds__(SEG_THREADS) void grad_mask_groups_kernel(uint32_t* __restrict__ g, int64_t n, int64_t bound, const int64_t* __restrict__ seg_off,
                                                                       const ishara_param_group* __restrict__ groups, int S, const int64_t* __restrict__ first) {
    const int64_t chunks = first[S] < bound ? first[S] : bound;
    uint4* __restrict__ g4 = reinterpret_cast<uint4*>(g);
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const AwpSpan p = awp_span(seg_off, first, S, n, c);
        if (groups[p.seg].frozen == 0) continue;
        const int64_t h = p.e0 + threadIdx.x, t = p.a1 + threadIdx.x;
        if (h < p.a0) g[h] = 0u;
        for (int64_t q = p.a0 / SEG_VEC + threadIdx.x; q < p.a1 / SEG_VEC; q += SEG_THREADS) g4[q] = make_uint4(0u, 0u, 0u, 0u);
        if (t < p.e1) g[t] = 0u;
    }
}

// ws: first int64 [S + 1], written by the setup launch of every call
int64_t param_groups_workspace_bytes(int64_t n, int32_t S) {
    if (n < 1 || S < 1 || S > n) return -1;
    return 8 * ((int64_t)S + 1);
}

int launch_radam_lookahead_groups(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n, RAdamArgs a, ishara_grad_stats* st,
                                  int skip, const int64_t* seg_off, const ishara_param_group* groups, int32_t S, void* ws, hipStream_t s) {
    int64_t* first = (int64_t*)ws;
    const int64_t bound = awp_chunk_bound(n, S);
    hipLaunchKernelGGL(awp_setup_kernel, dim3(1), dim3(SEG_THREADS), 0, s, seg_off, (int)S, first);
    if (launch_rc() != 0) return -2;
    if (st) hipLaunchKernelGGL(radam_lookahead_groups_kernel<true>, dim3(awp_grid(bound)), dim3(SEG_THREADS), 0, s, theta, grad, m, v, slow, n, bound, a, st, skip, seg_off, groups, (int)S, first);
    else hipLaunchKernelGGL(radam_lookahead_groups_kernel<false>, dim3(awp_grid(bound)), dim3(SEG_THREADS), 0, s, theta, grad, m, v, slow, n, bound, a, st, 0, seg_off, groups, (int)S, first);
    return launch_rc();
}

int launch_grad_mask_groups(float* g, int64_t n, const int64_t* seg_off, const ishara_param_group* groups, int32_t S, void* ws, hipStream_t s) {
    int64_t* first = (int64_t*)ws;
    const int64_t bound = awp_chunk_bound(n, S);
    hipLaunchKernelGGL(awp_setup_kernel, dim3(1), dim3(SEG_THREADS), 0, s, seg_off, (int)S, first);
    if (launch_rc() != 0) return -2;
    hipLaunchKernelGGL(grad_mask_groups_kernel, dim3(awp_grid(bound)), dim3(SEG_THREADS), 0, s, reinterpret_cast<uint32_t*>(g), n, bound, seg_off, groups, (int)S, first);
    return launch_rc();
}
