// Streaming kernels of adversarial weight perturbation (AWP): per-tensor norms of the flat fp32 gradient (and weights) over a caller's
// segment table, the perturbation w += scale[s] * g with a bit copy of the old weights kept aside, and the copy back.  Bound by HBM like
// grad_ops.hip and weight_avg.hip: 16-byte accesses wherever the addresses allow, no float atomics, every sum in a fixed order (results are
// bit-identical from run to run), no allocation, no synchronise, no memset: each launch writes every workspace word the next one reads.
//
// The trainable prefix [0, n) is cut by seg_off [S + 1] into S segments whose offsets are not 16-byte aligned in general.  Work is handed out
// in chunks of AWP_CHUNK elements that never cross a segment: segment s owns ceil(len_s / AWP_CHUNK) chunks, numbered consecutively.
//   awp_setup_kernel    one workgroup: first[s] = number of chunks in front of segment s, first[S] = all of them (<= n / AWP_CHUNK + S, the
//                       bound the host sizes the workspace and the grid from without reading the table)
//   awp_partial_kernel  chunk c -> part_g[c] (and part_w[c]): the fp64 sum of the squares of its elements
//   awp_finish_kernel   segment s: its chunks in index order -> ss_g (ss_w) -> scale[s], seg_ss[s], seg_zero[s]
//   awp_record_kernel   one workgroup: the 16-byte record from seg_ss / scale / seg_zero
//   awp_apply_kernel    the same chunks: backup = w (words), w = w + scale[s] * g unless the segment was zeroed
// A workgroup finds the segment of a chunk by bisection of first[] (wave-uniform loads of a table that stays in L2).
#include "seg_chunks.h"

// the chunk scheme lives in seg_chunks.h (the optimizer's parameter groups walk the same table); these are its constants under AWP's names
static constexpr int AWP_THREADS = SEG_THREADS;                // threads of a workgroup
static constexpr int AWP_VEC = SEG_VEC;                        // floats of one 16-byte access
static constexpr int AWP_CHUNK = 4096;                         // elements of a chunk (train_state.AWP_CHUNK): 4 x 16 bytes per thread
static constexpr int AWP_GRID_CAP = 2048;                      // most workgroups of a launch (train_state.GRAD_GRID_CAP)
static_assert(AWP_CHUNK == SEG_CHUNK && AWP_GRID_CAP == SEG_GRID_CAP, "awp.hip and seg_chunks.h disagree about the chunk scheme");

struct AwpWs { int64_t* first; double* seg_ss; int32_t* seg_zero; double* part_g; double* part_w; };

static inline int64_t awp_rup8(int64_t v) { return (v + 7) / 8 * 8; }
// first int64 [S + 1] | seg_ss double [S] | seg_zero int32 [S] (padded to 8 bytes) | part_g double [bound] | part_w double [bound]
int64_t awp_workspace_bytes(int64_t n, int32_t S) {
    if (n < 1 || S < 1 || S > n) return -1;
    return 8 * ((int64_t)S + 1) + 8 * (int64_t)S + awp_rup8(4 * (int64_t)S) + 16 * awp_chunk_bound(n, S);
}
static inline AwpWs awp_carve(void* ws, int64_t n, int32_t S) {
    char* p = (char*)ws;
    AwpWs a;
    a.first = (int64_t*)p;      p += 8 * ((int64_t)S + 1);
    a.seg_ss = (double*)p;      p += 8 * (int64_t)S;
    a.seg_zero = (int32_t*)p;   p += awp_rup8(4 * (int64_t)S);
    a.part_g = (double*)p;      p += 8 * awp_chunk_bound(n, S);
    a.part_w = (double*)p;
    return a;
}

__device__ __forceinline__ void awp_sq(float x, double& ss) { const double d = (double)x; ss += d * d; }      // squared in fp64: (3e19)^2 is past fp32

// fixed-order sum of the workgroup's 256 pairs -> thread 0 (called more than once per kernel: the barrier in front guards the reuse)
__device__ __forceinline__ void awp_block_sum(double& a, double& b) {
    __shared__ double s_a[AWP_THREADS / 64];
    __shared__ double s_b[AWP_THREADS / 64];
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o, 64);
        b += __shfl_down(b, o, 64);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = s_a[0]; b = s_b[0];
        for (int w = 1; w < AWP_THREADS / 64; ++w) { a += s_a[w]; b += s_b[w]; }
    }
}

// sum of squares of x over one chunk, this thread's share.  VEC: x is 16-byte aligned (w always is; g when the caller's pointer is)
template <bool VEC>
__device__ __forceinline__ double awp_chunk_sq(const float* __restrict__ x, const AwpSpan& p) {
    double ss = 0.0;
    if (VEC) {
        if (p.e0 + threadIdx.x < p.a0) awp_sq(x[p.e0 + threadIdx.x], ss);
        const float4* __restrict__ x4 = reinterpret_cast<const float4*>(x);
        for (int64_t v = p.a0 / AWP_VEC + threadIdx.x; v < p.a1 / AWP_VEC; v += AWP_THREADS) {
            const float4 q = x4[v];
            awp_sq(q.x, ss); awp_sq(q.y, ss); awp_sq(q.z, ss); awp_sq(q.w, ss);
        }
        if (p.a1 + threadIdx.x < p.e1) awp_sq(x[p.a1 + threadIdx.x], ss);
    } else {
        for (int64_t i = p.e0 + threadIdx.x; i < p.e1; i += AWP_THREADS) awp_sq(x[i], ss);
    }
    return ss;
}

template <bool G_VEC, bool RELATIVE>
__global__ __launch_bounds__(AWP_THREADS) void awp_partial_kernel(const float* __restrict__ w, const float* __restrict__ g, const int64_t* __restrict__ seg_off,
                                                                  int S, int64_t n, int64_t bound, const int64_t* __restrict__ first,
                                                                  double* __restrict__ part_g, double* __restrict__ part_w) {
    const int64_t chunks = first[S] < bound ? first[S] : bound;      // == first[S] for a table that keeps its contract
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const AwpSpan p = awp_span(seg_off, first, S, n, c);
        double sg = awp_chunk_sq<G_VEC>(g, p);
        double sw = RELATIVE ? awp_chunk_sq<true>(w, p) : 0.0;
        awp_block_sum(sg, sw);
        if (threadIdx.x == 0) { part_g[c] = sg; if (RELATIVE) part_w[c] = sw; }
    }
}

// segment s, one workgroup: thread t sums chunks t, t + 256, ... of the segment in index order, then the fixed-order workgroup sum.
// scale in fp64, rounded once.  A sum that is not finite (a NaN or Inf in the segment, or an overflow) zeroes the segment.
template <bool RELATIVE>
__global__ __launch_bounds__(AWP_THREADS) void awp_finish_kernel(const int64_t* __restrict__ first, int S, int64_t bound, const double* __restrict__ part_g,
                                                                 const double* __restrict__ part_w, float delta, float eps, float* __restrict__ scale,
                                                                 double* __restrict__ seg_ss, int32_t* __restrict__ seg_zero) {
    for (int s = blockIdx.x; s < S; s += gridDim.x) {
        const int64_t c1 = first[s + 1] < bound ? first[s + 1] : bound;
        double sg = 0.0, sw = 0.0;
        for (int64_t c = first[s] + threadIdx.x; c < c1; c += AWP_THREADS) { sg += part_g[c]; if (RELATIVE) sw += part_w[c]; }
        awp_block_sum(sg, sw);
        if (threadIdx.x == 0) {
            const bool zero = !isfinite(sg) || (RELATIVE && !isfinite(sw));
            float sc = 0.f;
            if (!zero) {
                const double den = sqrt(sg) + (double)eps;
                sc = RELATIVE ? (float)((double)delta * sqrt(sw) / den) : (float)((double)delta / den);
            }
            scale[s] = sc;
            seg_ss[s] = zero ? 0.0 : sg;
            seg_zero[s] = zero ? 1 : 0;
        }
    }
}

// one workgroup: thread t takes a contiguous run of segments in segment order, thread 0 adds the 256 run totals in order
__global__ __launch_bounds__(AWP_THREADS) void awp_record_kernel(int S, const float* __restrict__ scale, const double* __restrict__ seg_ss,
                                                                 const int32_t* __restrict__ seg_zero, ishara_awp_stats* __restrict__ rec) {
    __shared__ double s_g[AWP_THREADS];
    __shared__ double s_d[AWP_THREADS];
    __shared__ int s_z[AWP_THREADS];
    const int per = (S + AWP_THREADS - 1) / AWP_THREADS;
    const int lo = min((int64_t)threadIdx.x * per, (int64_t)S), hi = min((int64_t)lo + per, (int64_t)S);
    double sg = 0.0, sd = 0.0; int z = 0;
    for (int s = lo; s < hi; ++s) {
        if (seg_zero[s]) { ++z; continue; }
        const double sc = (double)scale[s];
        sg += seg_ss[s];
        sd += sc * sc * seg_ss[s];
    }
    s_g[threadIdx.x] = sg; s_d[threadIdx.x] = sd; s_z[threadIdx.x] = z;
    __syncthreads();
    if (threadIdx.x == 0) {
        sg = 0.0; sd = 0.0; z = 0;
        for (int t = 0; t < AWP_THREADS; ++t) { sg += s_g[t]; sd += s_d[t]; z += s_z[t]; }
        rec->grad_norm = (float)sqrt(sg);
        rec->delta_norm = (float)sqrt(sd);
        rec->perturbed = S - z;
        rec->zeroed = z;
    }
}

// w + scale * g in two fp32 roundings.  hipcc contracts a * b + c into an FMA by default, and __fmul_rn / __fadd_rn are plain operators in
// its headers, so they would fuse as well; the pragma takes the permission away (as weight_avg.hip's wavg_blend), which is what makes the
// numpy restatement (train_state.awp_reference) equal in every bit.
__device__ __forceinline__ uint32_t awp_step(uint32_t wbits, float g, float scale) {
#pragma clang fp contract(off)
    const float d = scale * g;
    const float r = __uint_as_float(wbits) + d;
    return __float_as_uint(r);
}

// the weights travel as 32-bit words: the copy into `backup` is exact for every pattern, NaN payloads included
template <bool G_VEC>
__global__ __launch_bounds__(AWP_THREADS) void awp_apply_kernel(uint32_t* __restrict__ w, uint32_t* __restrict__ backup, const float* __restrict__ g,
                                                                const int64_t* __restrict__ seg_off, int S, int64_t n, int64_t bound,
                                                                const int64_t* __restrict__ first, const float* __restrict__ scale,
                                                                const int32_t* __restrict__ seg_zero) {
    const int64_t chunks = first[S] < bound ? first[S] : bound;
    uint4* __restrict__ w4 = reinterpret_cast<uint4*>(w);
    uint4* __restrict__ b4 = reinterpret_cast<uint4*>(backup);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const AwpSpan p = awp_span(seg_off, first, S, n, c);
        const bool zero = seg_zero[p.seg] != 0;       // a zeroed segment: only the copy; neither g is read nor w written
        const float sc = scale[p.seg];
        const int64_t h = p.e0 + threadIdx.x, t = p.a1 + threadIdx.x;
        if (h < p.a0) { const uint32_t x = w[h]; backup[h] = x; if (!zero) w[h] = awp_step(x, g[h], sc); }
        for (int64_t v = p.a0 / AWP_VEC + threadIdx.x; v < p.a1 / AWP_VEC; v += AWP_THREADS) {
            uint4 x = w4[v];
            b4[v] = x;
            if (zero) continue;
            float4 q;
            if (G_VEC) q = g4[v];
            else { const float* gs = g + v * AWP_VEC; q.x = gs[0]; q.y = gs[1]; q.z = gs[2]; q.w = gs[3]; }
            x.x = awp_step(x.x, q.x, sc); x.y = awp_step(x.y, q.y, sc); x.z = awp_step(x.z, q.z, sc); x.w = awp_step(x.w, q.w, sc);
            w4[v] = x;
        }
        if (t < p.e1) { const uint32_t x = w[t]; backup[t] = x; if (!zero) w[t] = awp_step(x, g[t], sc); }
    }
}

int launch_awp_norms(const float* w, const float* g, const int64_t* seg_off, int32_t S, int64_t n, float delta, float eps, int relative, float* scale,
                     ishara_awp_stats* rec, void* ws, hipStream_t s) {
    const AwpWs a = awp_carve(ws, n, S);
    const int64_t bound = awp_chunk_bound(n, S);
    const int grid = awp_grid(bound);
    const bool gvec = (uintptr_t)g % 16 == 0;
    hipLaunchKernelGGL(awp_setup_kernel, dim3(1), dim3(AWP_THREADS), 0, s, seg_off, (int)S, a.first);
    if (launch_rc() != 0) return -2;
#define AWP_PARTIAL(GV, REL) hipLaunchKernelGGL((awp_partial_kernel<GV, REL>), dim3(grid), dim3(AWP_THREADS), 0, s, w, g, seg_off, (int)S, n, bound, a.first, a.part_g, a.part_w)
    if (relative) { if (gvec) AWP_PARTIAL(true, true); else AWP_PARTIAL(false, true); }
    else { if (gvec) AWP_PARTIAL(true, false); else AWP_PARTIAL(false, false); }
#undef AWP_PARTIAL
    if (launch_rc() != 0) return -2;
    if (relative) hipLaunchKernelGGL(awp_finish_kernel<true>, dim3(awp_grid(S)), dim3(AWP_THREADS), 0, s, a.first, (int)S, bound, a.part_g, a.part_w, delta, eps, scale, a.seg_ss, a.seg_zero);
    else hipLaunchKernelGGL(awp_finish_kernel<false>, dim3(awp_grid(S)), dim3(AWP_THREADS), 0, s, a.first, (int)S, bound, a.part_g, a.part_w, delta, eps, scale, a.seg_ss, a.seg_zero);
    if (launch_rc() != 0) return -2;
    hipLaunchKernelGGL(awp_record_kernel, dim3(1), dim3(AWP_THREADS), 0, s, (int)S, scale, a.seg_ss, a.seg_zero, rec);
    return launch_rc();
}

// behind launch_awp_norms on the same stream, with the same ws, seg_off, S and n
int launch_awp_apply(float* w, float* backup, const float* g, const int64_t* seg_off, int32_t S, int64_t n, const float* scale, void* ws, hipStream_t s) {
    const AwpWs a = awp_carve(ws, n, S);
    const int64_t bound = awp_chunk_bound(n, S);
    const int grid = awp_grid(bound);
    uint32_t* wu = reinterpret_cast<uint32_t*>(w);
    uint32_t* bu = reinterpret_cast<uint32_t*>(backup);
    if ((uintptr_t)g % 16 == 0) hipLaunchKernelGGL(awp_apply_kernel<true>, dim3(grid), dim3(AWP_THREADS), 0, s, wu, bu, g, seg_off, (int)S, n, bound, a.first, scale, a.seg_zero);
    else hipLaunchKernelGGL(awp_apply_kernel<false>, dim3(grid), dim3(AWP_THREADS), 0, s, wu, bu, g, seg_off, (int)S, n, bound, a.first, scale, a.seg_zero);
    return launch_rc();
}

// w = backup as 32-bit words
__global__ __launch_bounds__(AWP_THREADS) void awp_restore_kernel(uint32_t* __restrict__ w, const uint32_t* __restrict__ backup, int64_t n) {
    const int64_t n4 = n / AWP_VEC, stride = (int64_t)gridDim.x * AWP_THREADS;
    uint4* __restrict__ w4 = reinterpret_cast<uint4*>(w);
    const uint4* __restrict__ b4 = reinterpret_cast<const uint4*>(backup);
    for (int64_t i = (int64_t)blockIdx.x * AWP_THREADS + threadIdx.x; i < n4; i += stride) w4[i] = b4[i];
    const int64_t e = n4 * AWP_VEC + threadIdx.x;
    if (blockIdx.x == 0 && e < n) w[e] = backup[e];
}

int launch_awp_restore(float* w, const float* backup, int64_t n, hipStream_t s) {
    const int grid = awp_grid((n + (int64_t)AWP_THREADS * AWP_VEC - 1) / ((int64_t)AWP_THREADS * AWP_VEC));
    hipLaunchKernelGGL(awp_restore_kernel, dim3(grid), dim3(AWP_THREADS), 0, s, reinterpret_cast<uint32_t*>(w), reinterpret_cast<const uint32_t*>(backup), n);
    return launch_rc();
}
