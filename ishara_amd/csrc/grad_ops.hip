// Streaming kernels over the flat fp32 gradient: global-norm statistics (norm, clip coefficient, non-finite count) and the
// microbatch accumulator.  Both are bound by HBM: 16-byte loads and stores, a grid sized from the element count with a fixed cap, no
// float atomics, every sum taken in a fixed order (results are bit-identical from run to run), no allocation, no synchronise.
#include "kernels.h"

static constexpr int GRAD_THREADS = 256;                       // threads of a workgroup
static constexpr int GRAD_VEC = 4;                             // floats of one 16-byte access
static constexpr int GRAD_WG_SPAN = GRAD_THREADS * GRAD_VEC;   // elements one workgroup covers per grid-stride round (train_state.GRAD_WG_SPAN)
static constexpr int GRAD_GRID_CAP = 2048;                     // most workgroups of a launch (train_state.GRAD_GRID_CAP): 256 CUs x 8
struct GradPartial { double sumsq; int64_t nonfinite; };       // one workspace row per workgroup

static inline int grad_grid(int64_t n) {
    const int64_t g = (n + GRAD_WG_SPAN - 1) / GRAD_WG_SPAN;
    return (int)(g < GRAD_GRID_CAP ? g : GRAD_GRID_CAP);
}
int64_t grad_stats_workspace_bytes(int64_t n) { return n < 1 ? -1 : (int64_t)sizeof(GradPartial) * grad_grid(n); }

__device__ __forceinline__ void grad_stats_take(float x, double& ss, int& bad) {
    const double d = (double)x;             // squared in fp64: (3e19)^2 is past fp32
    ss += d * d;
    bad += (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1 : 0;      // NaN or +-Inf
}

// fixed-order sum of the workgroup's 256 (ss, bad) pairs -> thread 0
__device__ __forceinline__ void grad_block_sum(double& ss, int64_t& bad) {
    __shared__ double s_ss[GRAD_THREADS / 64];
    __shared__ int64_t s_bad[GRAD_THREADS / 64];
    for (int o = 32; o > 0; o >>= 1) {
        ss += __shfl_down(ss, o, 64);
        bad += __shfl_down(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_ss[threadIdx.x >> 6] = ss; s_bad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ss = s_ss[0]; bad = s_bad[0];
        for (int w = 1; w < GRAD_THREADS / 64; ++w) { ss += s_ss[w]; bad += s_bad[w]; }
    }
}

// pass 1: workgroup b sums the squares and counts the non-finite elements of its grid-stride share of g into row b of the workspace
__global__ __launch_bounds__(GRAD_THREADS) void grad_stats_partial_kernel(const float* __restrict__ g, int64_t n, GradPartial* __restrict__ part) {
    const int64_t n4 = n / GRAD_VEC, stride = (int64_t)gridDim.x * GRAD_THREADS;
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    double ss = 0.0; int bad = 0;       // a thread sees at most n / (4 * 256) + 3 < 2^21 + 3 elements
    for (int64_t i = (int64_t)blockIdx.x * GRAD_THREADS + threadIdx.x; i < n4; i += stride) {
        const float4 v = g4[i];
        grad_stats_take(v.x, ss, bad); grad_stats_take(v.y, ss, bad); grad_stats_take(v.z, ss, bad); grad_stats_take(v.w, ss, bad);
    }
    if (blockIdx.x == 0 && n4 * GRAD_VEC + threadIdx.x < n) grad_stats_take(g[n4 * GRAD_VEC + threadIdx.x], ss, bad);      // the n % 4 last elements
    int64_t bad64 = bad;
    grad_block_sum(ss, bad64);
    if (threadIdx.x == 0) { part[blockIdx.x].sumsq = ss; part[blockIdx.x].nonfinite = bad64; }
}

// pass 2, one workgroup: the rows in a fixed order -> norm, coef, nonfinite (`skipped` is left alone: the optimizer step owns it)
__global__ __launch_bounds__(GRAD_THREADS) void grad_stats_finish_kernel(const GradPartial* __restrict__ part, int rows, float grad_scale, float clip_norm,
                                                                         ishara_grad_stats* __restrict__ out) {
    double ss = 0.0; int64_t bad = 0;
    for (int r = threadIdx.x; r < rows; r += GRAD_THREADS) { ss += part[r].sumsq; bad += part[r].nonfinite; }
    grad_block_sum(ss, bad);
    if (threadIdx.x == 0) {
        const float norm = (float)((double)grad_scale * sqrt(ss));
        float coef = grad_scale;
        if (clip_norm > 0.f) coef = grad_scale * fminf(1.f, clip_norm / (norm + 1e-6f));      // torch.nn.utils.clip_grad_norm_
        out->norm = norm;
        out->coef = coef;
        out->nonfinite = bad > 0x7fffffffLL ? 0x7fffffff : (int32_t)bad;
    }
}

int launch_grad_stats(const float* g, int64_t n, float grad_scale, float clip_norm, ishara_grad_stats* out, void* ws, hipStream_t s) {
    const int grid = grad_grid(n);
    GradPartial* part = (GradPartial*)ws;
    hipLaunchKernelGGL(grad_stats_partial_kernel, dim3(grid), dim3(GRAD_THREADS), 0, s, g, n, part);
    if (launch_rc() != 0) return -2;
    hipLaunchKernelGGL(grad_stats_finish_kernel, dim3(1), dim3(GRAD_THREADS), 0, s, part, grid, grad_scale, clip_norm, out);
    return launch_rc();
}

// acc[i] = first ? g[i] : acc[i] + g[i]: one fp32 add per element, so k calls leave the left-to-right fp32 sum
template <bool FIRST>
__global__ __launch_bounds__(GRAD_THREADS) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, int64_t n) {
    const int64_t n4 = n / GRAD_VEC, stride = (int64_t)gridDim.x * GRAD_THREADS;
    float4* __restrict__ a4 = reinterpret_cast<float4*>(acc);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    for (int64_t i = (int64_t)blockIdx.x * GRAD_THREADS + threadIdx.x; i < n4; i += stride) {
        float4 v = g4[i];
        if (!FIRST) { const float4 a = a4[i]; v.x = a.x + v.x; v.y = a.y + v.y; v.z = a.z + v.z; v.w = a.w + v.w; }
        a4[i] = v;
    }
    const int64_t t = n4 * GRAD_VEC + threadIdx.x;
    if (blockIdx.x == 0 && t < n) acc[t] = FIRST ? g[t] : acc[t] + g[t];
}

int launch_grad_accumulate(float* acc, const float* g, int64_t n, int first, hipStream_t s) {
    const int grid = grad_grid(n);
    if (first) hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3(grid), dim3(GRAD_THREADS), 0, s, acc, g, n);
    else hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3(grid), dim3(GRAD_THREADS), 0, s, acc, g, n);
    return launch_rc();
}
