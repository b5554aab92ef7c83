// Streaming kernels of the exponential moving average of the weights (Keras use_ema / ema_momentum / ema_overwrite_frequency): the update
// of the average behind an optimizer step, and the bit-for-bit exchange of two buffers that swaps the average in for evaluation.  Built
// like grad_ops.hip: 256 threads, 16-byte accesses, a grid sized from the element count with the same fixed cap, the n % 4 last elements
// by the first threads of workgroup 0, no atomics, no allocation, no synchronise.
#include "kernels.h"

static constexpr int WAVG_THREADS = 256;                       // threads of a workgroup
static constexpr int WAVG_VEC = 4;                             // floats of one 16-byte access
static constexpr int WAVG_WG_SPAN = WAVG_THREADS * WAVG_VEC;   // elements one workgroup covers per grid-stride round (train_state.GRAD_WG_SPAN)
static constexpr int WAVG_GRID_CAP = 2048;                     // most workgroups of a launch (train_state.GRAD_GRID_CAP)

static inline int wavg_grid(int64_t n) {
    const int64_t g = (n + WAVG_WG_SPAN - 1) / WAVG_WG_SPAN;
    return (int)(g < WAVG_GRID_CAP ? g : WAVG_GRID_CAP);
}

struct WavgPlan { float alpha; int skip; int overwrite; };

// What one launch does, from the two device records alone (every thread of both kernels derives the same plan; nothing in it depends on a
// host value that changes from step to step, so a captured graph replays correctly).  alpha = (float)(1 - d) with d = momentum, under
// warm-up min(momentum, (1 + n) / (10 + n)) (the num_updates rule of tf.train.ExponentialMovingAverage), all in fp64; n = updates so far.
__device__ __forceinline__ WavgPlan wavg_plan(const ishara_ema_state* rec, const ishara_grad_stats* st, int skip, float momentum, int warmup, int every) {
    WavgPlan p;
    p.skip = (skip && st->nonfinite > 0) ? 1 : 0;
    const int64_t n = rec->updates;
    double d = (double)momentum;
    if (warmup) d = fmin(d, (1.0 + (double)n) / (10.0 + (double)n));
    p.alpha = (float)(1.0 - d);
    p.overwrite = (every > 0 && (n + 1) % every == 0) ? 1 : 0;
    return p;
}

// avg + alpha * (theta - avg) in three fp32 roundings.  hipcc contracts a * b + c into an FMA by default, and __fmul_rn / __fadd_rn are
// plain operators in its headers, so they would fuse as well; the pragma takes the permission away from these three operations, which
// is what makes the numpy fp32 restatement (train_state.ema_reference) equal in every bit.
__device__ __forceinline__ float wavg_blend(float a, float t, float alpha) {
#pragma clang fp contract(off)
    const float diff = t - a;
    const float step = alpha * diff;
    return a + step;
}

// Every workgroup reads rec->updates (and st->nonfinite), none writes the record: see weight_average_commit_kernel.
template <bool MAY_OVERWRITE>
__global__ __launch_bounds__(WAVG_THREADS) void weight_average_kernel(float* __restrict__ avg, float* __restrict__ theta, int64_t n, float momentum, int warmup,
                                                                      int every, const ishara_ema_state* __restrict__ rec,
                                                                      const ishara_grad_stats* __restrict__ st, int skip) {
    const WavgPlan p = wavg_plan(rec, st, skip, momentum, warmup, MAY_OVERWRITE ? every : 0);
    if (p.skip) return;       // the optimizer wrote nothing: neither does the average
    const int64_t n4 = n / WAVG_VEC, stride = (int64_t)gridDim.x * WAVG_THREADS;
    float4* __restrict__ a4 = reinterpret_cast<float4*>(avg);
    float4* __restrict__ t4 = reinterpret_cast<float4*>(theta);
    for (int64_t i = (int64_t)blockIdx.x * WAVG_THREADS + threadIdx.x; i < n4; i += stride) {
        float4 a = a4[i];
        const float4 t = t4[i];
        a.x = wavg_blend(a.x, t.x, p.alpha); a.y = wavg_blend(a.y, t.y, p.alpha); a.z = wavg_blend(a.z, t.z, p.alpha); a.w = wavg_blend(a.w, t.w, p.alpha);
        a4[i] = a;
        if (MAY_OVERWRITE && p.overwrite) t4[i] = a;
    }
    const int64_t e = n4 * WAVG_VEC + threadIdx.x;
    if (blockIdx.x == 0 && e < n) {
        const float a = wavg_blend(avg[e], theta[e], p.alpha);
        avg[e] = a;
        if (MAY_OVERWRITE && p.overwrite) theta[e] = a;
    }
}

// The record of the launch, by one thread in a launch of its own behind the update.  A workgroup of the update kernel must not advance
// `updates`: the workgroups of a grid do not start together (a grid-stride launch of 2048 workgroups runs in several waves on the chip),
// so one that starts late would read the advanced counter and take another alpha and another overwrite decision than the early ones.
// The stream orders this launch behind all of them, as grad_stats_finish_kernel runs behind grad_stats_partial_kernel.
__global__ void weight_average_commit_kernel(float momentum, int warmup, int every, ishara_ema_state* rec, const ishara_grad_stats* st, int skip) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const WavgPlan p = wavg_plan(rec, st, skip, momentum, warmup, every);
    if (p.skip) { rec->overwrote = 0; return; }       // updates and alpha keep their values
    rec->alpha = p.alpha;
    rec->overwrote = p.overwrite;
    rec->updates = rec->updates + 1;
}

int launch_weight_average(float* avg, float* theta, int64_t n, float momentum, int warmup, int overwrite_every, ishara_ema_state* rec,
                          const ishara_grad_stats* st, int skip, hipStream_t s) {
    const int grid = wavg_grid(n);
    if (overwrite_every > 0)
        hipLaunchKernelGGL(weight_average_kernel<true>, dim3(grid), dim3(WAVG_THREADS), 0, s, avg, theta, n, momentum, warmup, overwrite_every, rec, st, skip);
    else
        hipLaunchKernelGGL(weight_average_kernel<false>, dim3(grid), dim3(WAVG_THREADS), 0, s, avg, theta, n, momentum, warmup, 0, rec, st, skip);
    if (launch_rc() != 0) return -2;
    hipLaunchKernelGGL(weight_average_commit_kernel, dim3(1), dim3(1), 0, s, momentum, warmup, overwrite_every, rec, st, skip);
    return launch_rc();
}

// a <-> b as 32-bit words: no float operation touches the data, so NaN payloads and signalling NaNs travel unchanged
__global__ __launch_bounds__(WAVG_THREADS) void weight_swap_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, int64_t n) {
    const int64_t n4 = n / WAVG_VEC, stride = (int64_t)gridDim.x * WAVG_THREADS;
    uint4* __restrict__ a4 = reinterpret_cast<uint4*>(a);
    uint4* __restrict__ b4 = reinterpret_cast<uint4*>(b);
    for (int64_t i = (int64_t)blockIdx.x * WAVG_THREADS + threadIdx.x; i < n4; i += stride) {
        const uint4 x = a4[i], y = b4[i];
        a4[i] = y;
        b4[i] = x;
    }
    const int64_t e = n4 * WAVG_VEC + threadIdx.x;
    if (blockIdx.x == 0 && e < n) { const uint32_t x = a[e], y = b[e]; a[e] = y; b[e] = x; }
}

int launch_weight_swap(float* a, float* b, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(weight_swap_kernel, dim3(wavg_grid(n)), dim3(WAVG_THREADS), 0, s, reinterpret_cast<uint32_t*>(a), reinterpret_cast<uint32_t*>(b), n);
    return launch_rc();
}
