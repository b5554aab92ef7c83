// Sums of split partial rows ("slabs"): out[i] += sum_s slab[s * stride + i].  Used by the weight-gradient GEMMs and by the
// LayerNorm and depthwise-conv backward passes for their parameter gradients; single launches, or deferred through a RedSink.
#include "kernels.h"

// out[i] += sum_s slab[s*stride + i].  grid = (n/4/256, split groups): each block sums its
// subset of splits with 4 independent 16-byte loads in flight and issues one atomic per element.
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ slab, float* __restrict__ out, int n, int splits, size_t stride) {
    const int i4 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i4 >= n) return;
    const int per = (splits + gridDim.y - 1) / gridDim.y;
    const int s0 = blockIdx.y * per, s1 = min(splits, s0 + per);
    if (i4 + 4 <= n && (stride & 3) == 0) {
        float4 acc[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        int sidx = s0;
        for (; sidx + 8 <= s1; sidx += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float4 v = *reinterpret_cast<const float4*>(slab + (size_t)(sidx + u) * stride + i4);
                acc[u].x += v.x; acc[u].y += v.y; acc[u].z += v.z; acc[u].w += v.w;
            }
        }
        for (; sidx < s1; ++sidx) {
            const float4 v = *reinterpret_cast<const float4*>(slab + (size_t)sidx * stride + i4);
            acc[0].x += v.x; acc[0].y += v.y; acc[0].z += v.z; acc[0].w += v.w;
        }
#pragma unroll
        for (int u = 1; u < 8; ++u) { acc[0].x += acc[u].x; acc[0].y += acc[u].y; acc[0].z += acc[u].z; acc[0].w += acc[u].w; }
        if (gridDim.y == 1) {
            float4 o = *reinterpret_cast<const float4*>(out + i4);
            o.x += acc[0].x; o.y += acc[0].y; o.z += acc[0].z; o.w += acc[0].w;
            *reinterpret_cast<float4*>(out + i4) = o;
        } else {
            atomicAdd(out + i4, acc[0].x); atomicAdd(out + i4 + 1, acc[0].y);
            atomicAdd(out + i4 + 2, acc[0].z); atomicAdd(out + i4 + 3, acc[0].w);
        }
    } else {
        for (int e = 0; e < 4 && i4 + e < n; ++e) {
            float acc = 0.f;
            for (int sidx = s0; sidx < s1; ++sidx) acc += slab[(size_t)sidx * stride + i4 + e];
            atomicAdd(out + i4 + e, acc);
        }
    }
}

// Slab sums without atomics: a workgroup of 256 threads owns 4*CQ columns; thread (cq = tid % CQ, sl = tid / CQ) sums the
// slabs sl, sl+SL, ... of column quad cq with 8 loads in flight (SL = 8 covers 64 splits in one pass), the SL partial
// rows are combined through LDS in a fixed order, and ONE thread adds the total to out; one launch serves two outputs
// (columns [0, n0) -> out0, [n0, n) -> out1).  Same-address atomics were the whole cost of the first reducer (2-way 80 us,
// 4-way 83 us, 8-way 106 us per wgrad including the GEMM); 128 slab lanes with one load each ran 10.5 us per 32 MB.
template <int SL, int CQ>
__global__ __launch_bounds__(SL * CQ) void reduce_slabs_cols_kernel(const float* __restrict__ slab, float* __restrict__ out0, float* __restrict__ out1,
                                                                    int n0, int n, int splits, size_t stride, int nb, int nbv) {
    __shared__ float4 red[SL][CQ];
    const int tid = threadIdx.x, cq = tid % CQ, sl = tid / CQ;
    const int col = blockIdx.x * (CQ * 4) + cq * 4;
    // nb != 0: the slab rows are nb wide with only the first nbv columns real (zero-padded B operand); out0 rows are nbv wide
    const int cin = nb ? (col < n0 ? col % nb : col - n0) : 0;
    const bool valid = col < n && (nb == 0 || cin < nbv);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
        for (int s0 = sl; s0 < splits; s0 += SL * 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int sidx = s0 + SL * u;
                v[u] = sidx < splits ? *reinterpret_cast<const float4*>(slab + (size_t)sidx * stride + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
        }
    }
    red[sl][cq] = acc;
    __syncthreads();
    if (sl == 0 && valid) {
        float4 t = red[0][cq];
#pragma unroll
        for (int w = 1; w < SL; ++w) { t.x += red[w][cq].x; t.y += red[w][cq].y; t.z += red[w][cq].z; t.w += red[w][cq].w; }
        float* dst = col < n0 ? (nb ? out0 + (size_t)(col / nb) * nbv + cin : out0 + col) : out1 + (col - n0);      // parameter blocks of the flat gradient are only 4-byte aligned
        dst[0] += t.x; dst[1] += t.y; dst[2] += t.z; dst[3] += t.w;
    }
}
static void launch_reduce_cols(const float* slab, float* out0, float* out1, int n0, int n, int splits, size_t stride, hipStream_t s, int nb = 0, int nbv = 0) {
    if (n <= 2048) hipLaunchKernelGGL((reduce_slabs_cols_kernel<64, 4>), dim3((n + 15) / 16), dim3(256), 0, s, slab, out0, out1, n0, n, splits, stride, nb, nbv);   // narrow, many partial rows (LayerNorm, dwconv)
    else if (splits <= 64) hipLaunchKernelGGL((reduce_slabs_cols_kernel<8, 32>), dim3((n + 127) / 128), dim3(256), 0, s, slab, out0, out1, n0, n, splits, stride, nb, nbv);
    else hipLaunchKernelGGL((reduce_slabs_cols_kernel<16, 16>), dim3((n + 63) / 64), dim3(256), 0, s, slab, out0, out1, n0, n, splits, stride, nb, nbv);
}

bool reduce_cols_ok(const float* slab, const float* out0, const float* out1, int n0, int n, size_t stride) {
    (void)out0; (void)out1;
    return n % 4 == 0 && n0 % 4 == 0 && stride % 4 == 0 && ((uintptr_t)slab) % 16 == 0;
}

// ---- the deferred form: every recorded job in one launch.  A workgroup = 16 slab lanes x 16 column quads (64 columns of one job); the jobs'
// first block indices ride in the kernel arguments (scalar loads), the body is reduce_slabs_cols_kernel<16, 16>'s.
RedSink* g_red_sink = nullptr;
struct RedBatch { RedJob job[RED_MAXJOBS]; int njobs; };
__global__ __launch_bounds__(256) void reduce_jobs_kernel(RedBatch b) {
    constexpr int SL = 16, CQ = 16;
    __shared__ float4 red[SL][CQ];
    int j = 0;
    for (int t = 1; t < b.njobs; ++t) if ((int)blockIdx.x >= b.job[t].first_block) j = t;      // uniform: scalar compares
    const RedJob J = b.job[j];
    const int tid = threadIdx.x, cq = tid % CQ, sl = tid / CQ;
    const int col = ((int)blockIdx.x - J.first_block) * (CQ * 4) + cq * 4;
    const int cin = J.nb ? (col < J.n0 ? col % J.nb : col - J.n0) : 0;
    const bool valid = col < J.n && (J.nb == 0 || cin < J.nbv);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
        for (int s0 = sl; s0 < J.splits; s0 += SL * 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int sidx = s0 + SL * u;
                v[u] = sidx < J.splits ? *reinterpret_cast<const float4*>(J.slab + (size_t)sidx * J.stride + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
        }
    }
    red[sl][cq] = acc;
    __syncthreads();
    if (sl == 0 && valid) {
        float4 t = red[0][cq];
#pragma unroll
        for (int w = 1; w < SL; ++w) { t.x += red[w][cq].x; t.y += red[w][cq].y; t.z += red[w][cq].z; t.w += red[w][cq].w; }
        float* dst = col < J.n0 ? (J.nb ? J.out0 + (size_t)(col / J.nb) * J.nbv + cin : J.out0 + col) : J.out1 + (col - J.n0);
        dst[0] += t.x; dst[1] += t.y; dst[2] += t.z; dst[3] += t.w;
    }
}
bool reduce_sink_full() { return g_red_sink && g_red_sink->njobs >= RED_MAXJOBS - 2; }
static bool reduce_sink_take(const float* slab, float* out0, float* out1, int n0, int n, int splits, size_t stride, int nb, int nbv) {
    RedSink* k = g_red_sink;
    if (!k || k->njobs >= RED_MAXJOBS || !reduce_cols_ok(slab, out0, out1, n0, n, stride)) return false;
    // two jobs into the same parameter (the Conformer block's shared layer_norm1 is differentiated twice) would add to it from two workgroups
    // of the one launch: the later one is launched on its own right away, the batch follows in stream order (two ordered adds)
    for (int i = 0; i < k->njobs; ++i)
        if (k->job[i].out0 == out0 || (out1 && k->job[i].out1 == out1) || (out1 && k->job[i].out0 == out1) || k->job[i].out1 == out0) return false;
    RedJob& J = k->job[k->njobs++];
    J.slab = slab; J.out0 = out0; J.out1 = out1; J.stride = stride; J.n0 = n0; J.n = n; J.splits = splits; J.nb = nb; J.nbv = nbv;
    J.first_block = k->nblocks;
    k->nblocks += (n + 63) / 64;
    return true;
}
int launch_reduce_flush(RedSink* sink, hipStream_t s) {
    if (!sink || sink->njobs == 0) return 0;
    RedBatch b;
    for (int i = 0; i < sink->njobs; ++i) b.job[i] = sink->job[i];
    b.njobs = sink->njobs;
    hipLaunchKernelGGL(reduce_jobs_kernel, dim3(sink->nblocks), dim3(256), 0, s, b);
    sink->njobs = 0; sink->nblocks = 0;
    return launch_rc();
}

// out0[0..n0) += column sums of slab[:, 0..n0), out1[0..n1) += column sums of slab[:, n0..n0+n1)   (slab rows `stride` floats apart)
void launch_reduce_slabs2(const float* slab, float* out0, int n0, float* out1, int n1, int splits, size_t stride, hipStream_t s, int nb, int nbv) {
    if (reduce_sink_take(slab, out0, out1, n0, n0 + n1, splits, stride, nb, nbv)) return;
    if (reduce_cols_ok(slab, out0, out1, n0, n0 + n1, stride)) { launch_reduce_cols(slab, out0, out1, n0, n0 + n1, splits, stride, s, nb, nbv); return; }
    launch_reduce_slabs(slab, out0, n0, splits, stride, s);
    if (out1 && n1 > 0) launch_reduce_slabs(slab + n0, out1, n1, splits, stride, s);
}

void launch_reduce_slabs(const float* slab, float* out, int n, int splits, size_t stride, hipStream_t s) {
    if (reduce_sink_take(slab, out, nullptr, n, n, splits, stride, 0, 0)) return;
    if (reduce_cols_ok(slab, out, nullptr, n, n, stride)) { launch_reduce_cols(slab, out, nullptr, n, n, splits, stride, s); return; }
    const int gx = (n + 1023) / 1024;
    int gy = 1;                                            // split groups: enough workgroups to fill the chip
    while (gx * gy < 256 && gy * 16 <= splits) gy *= 2;     // same-address atomics are expensive: 8-way 106 us, 4-way 83 us per wgrad (incl. GEMM)
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(gx, gy), dim3(256), 0, s, slab, out, n, splits, stride);
}
