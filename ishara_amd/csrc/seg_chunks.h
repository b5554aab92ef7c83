// The chunk scheme over a segment table, shared by awp.hip and the parameter groups of optimizer.hip.
//
// The trainable prefix [0, n) is cut by seg_off [S + 1] into S segments whose offsets are not 16-byte aligned in general.  Work is handed out
// in chunks of SEG_CHUNK elements that never cross a segment: segment s owns ceil(len_s / SEG_CHUNK) chunks, numbered consecutively.
//   awp_setup_kernel    one workgroup: first[s] = number of chunks in front of segment s, first[S] = all of them (<= n / SEG_CHUNK + S, the
//                       bound the host sizes the workspace and the grid from without reading the table)
// A workgroup finds the segment of a chunk by bisection of first[] (wave-uniform loads of a table that stays in L2).
#pragma once
#include "kernels.h"

static constexpr int SEG_THREADS = 256;                        // threads of a workgroup
static constexpr int SEG_VEC = 4;                              // floats of one 16-byte access
static constexpr int SEG_CHUNK = 4096;                         // elements of a chunk (train_state.AWP_CHUNK): 4 x 16 bytes per thread
static constexpr int SEG_GRID_CAP = 2048;                      // most workgroups of a launch (train_state.GRAD_GRID_CAP)

static inline int64_t awp_chunk_bound(int64_t n, int64_t S) { return (n + SEG_CHUNK - 1) / SEG_CHUNK + S; }
static inline int awp_grid(int64_t work) { return (int)(work < SEG_GRID_CAP ? (work < 1 ? 1 : work) : SEG_GRID_CAP); }

__device__ __forceinline__ int64_t awp_chunks_of(int64_t len) { return (len + SEG_CHUNK - 1) / SEG_CHUNK; }

// exclusive prefix of the chunk counts: thread t takes a contiguous run of segments, thread 0 scans the 256 run totals
static __global__ __launch_bounds__(SEG_THREADS) void awp_setup_kernel(const int64_t* __restrict__ seg_off, int S, int64_t* __restrict__ first) {
    __shared__ int64_t s_run[SEG_THREADS];
    const int per = (S + SEG_THREADS - 1) / SEG_THREADS;
    const int lo = min((int64_t)threadIdx.x * per, (int64_t)S), hi = min((int64_t)lo + per, (int64_t)S);
    int64_t tot = 0;
    for (int s = lo; s < hi; ++s) tot += awp_chunks_of(seg_off[s + 1] - seg_off[s]);
    s_run[threadIdx.x] = tot;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t acc = 0;
        for (int t = 0; t < SEG_THREADS; ++t) { const int64_t r = s_run[t]; s_run[t] = acc; acc += r; }
        first[S] = acc;
    }
    __syncthreads();
    int64_t acc = s_run[threadIdx.x];
    for (int s = lo; s < hi; ++s) { first[s] = acc; acc += awp_chunks_of(seg_off[s + 1] - seg_off[s]); }
}

// the segment that owns chunk c: the largest s with first[s] <= c (first is strictly increasing: every segment has a chunk)
__device__ __forceinline__ int awp_segment_of(const int64_t* __restrict__ first, int S, int64_t c) {
    int lo = 0, hi = S;                 // first[lo] <= c < first[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (first[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// The elements [e0, e1) of chunk c, cut where 16-byte accesses begin and end: [e0, a0) head, [a0, a1) whole float4s, [a1, e1) tail.
// The buffers' base addresses are 16-byte aligned, so element i is on a 16-byte boundary when i % 4 == 0.
struct AwpSpan { int64_t e0, a0, a1, e1; int seg; };
__device__ __forceinline__ AwpSpan awp_span(const int64_t* __restrict__ seg_off, const int64_t* __restrict__ first, int S, int64_t n, int64_t c) {
    AwpSpan p;
    p.seg = awp_segment_of(first, S, c);
    const int64_t end = seg_off[p.seg + 1] < n ? seg_off[p.seg + 1] : n;      // a table that keeps its contract never needs the clamps: they
    p.e0 = seg_off[p.seg] + (c - first[p.seg]) * SEG_CHUNK;                     // keep one that does not inside [0, n)
    if (p.e0 < 0) p.e0 = 0;
    p.e1 = p.e0 + SEG_CHUNK < end ? p.e0 + SEG_CHUNK : end;
    if (p.e1 < p.e0) p.e1 = p.e0;
    p.a0 = (p.e0 + SEG_VEC - 1) / SEG_VEC * SEG_VEC;
    if (p.a0 > p.e1) p.a0 = p.e1;
    p.a1 = p.e1 / SEG_VEC * SEG_VEC;
    if (p.a1 < p.a0) p.a1 = p.a0;
    return p;
}
