// Inference-side preprocessing of the reference's TFLite wrapper (conv-hybrid-model.ipynb c3:61-115, c13:9-15) as ONE
// kernel: frame filter (hand present or even frame), NaN-pad / bilinear resize over time to T frames,
// per-landmark normalisation, [T,92,3] -> [T,276] re-ordering, NaN -> 0.  The clip length is read from device memory so
// the launch can live inside a captured hipGraph.
#include "preprocess_common.h"

// grid = PP_BLOCKS workgroups: every workgroup builds the (cheap) frame list again and writes its slice of the output — as ONE workgroup
// with a serial compaction by thread 0 the kernel took 83 us of a 1.3 ms clip (configs[4]).
#define PP_BLOCKS 24
__global__ __launch_bounds__(1024) void preprocess_kernel(const float* __restrict__ raw, const int* __restrict__ n_frames_p, int max_frames,
                                                          const float* __restrict__ mean, const float* __restrict__ stdv,
                                                          float* __restrict__ out, int Tn) {
    extern __shared__ int sh[];            // compacted source index list [max_frames]
    __shared__ int s_wcnt[16], s_base;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int n = *n_frames_p;
    n = n < 0 ? 0 : (n > max_frames ? max_frames : n);
    // ---- frame mask: any hand landmark present (NaN -> 0, sum != 0) or even frame (c3:89-93); kept frames are compacted in order by a
    // ballot prefix (1024 frames per round)
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int f0 = 0; f0 < n; f0 += 1024) {
        const int f = f0 + tid;
        int keep = 0;
        if (f < n) {
            float sacc = 0.f;
            for (int a = 0; a < 3; ++a)
                for (int j = 0; j < 42; ++j) { const float v = raw[(size_t)f * PP_COLS + a * PP_LM + j]; sacc += (v != v) ? 0.f : v; }
            keep = (sacc != 0.f || (f & 1) == 0) ? 1 : 0;
        }
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcnt[wid] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wid; ++w) off += s_wcnt[w];
        if (keep) sh[off + before] = f;
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < 16; ++w) t += s_wcnt[w]; s_base += t; }
        __syncthreads();
    }
    const int m = s_base;
    const float ratio = m > 0 ? (float)m / (float)Tn : 1.f;
    for (int i = blockIdx.x * blockDim.x + tid; i < Tn * PP_COLS; i += gridDim.x * blockDim.x) {
        const int t = i / PP_COLS, c = i - t * PP_COLS;
        out[i] = pp_value(raw, sh, n, m, Tn, ratio, t, c, mean, stdv);
    }
}

int launch_preprocess(const float* raw, const int* n_frames, int max_frames, const float* mean, const float* stdv, float* out, int T, hipStream_t s) {
    hipLaunchKernelGGL(preprocess_kernel, dim3(PP_BLOCKS), dim3(1024), (size_t)max_frames * sizeof(int), s, raw, n_frames, max_frames, mean, stdv, out, T);
    return launch_rc();
}

// ---- batched ragged form: B clips packed back to back in raw [N_total,276] (16-byte aligned), clip b = rows [offsets[b], offsets[b+1])
// of a device-resident int64 table (graph-capturable), out [B,T,276] (16-byte aligned).  Grid (k, B): the k workgroups of a clip each
// rebuild its kept-frame list in LDS (only the odd frames are tested: even frames are always kept) and write every k-th float4 of its
// T*276 outputs through pp_value, so every element is bit-identical to preprocess_kernel's for the same clip.
#define PPB_THREADS 256

// the hand-present test of one frame is pp_hand_present (preprocess_common.h): the sum in preprocess_kernel's order, read as float4 / float2

__global__ __launch_bounds__(PPB_THREADS) void preprocess_batch_kernel(const float* __restrict__ raw, int64_t n_total, const int64_t* __restrict__ offsets,
                                                                       int max_frames, const float* __restrict__ mean, const float* __restrict__ stdv,
                                                                       float* __restrict__ out, int Tn) {
    extern __shared__ int sh[];            // compacted source index list [max_frames]
    __shared__ int s_wcnt[PPB_THREADS / WAVE], s_base;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, b = blockIdx.y;
    // clip rows, clamped to the packed buffer: a bad table cannot make the kernel read outside raw
    int64_t lo = offsets[b], hi = offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > n_total ? n_total : lo);
    hi = hi < lo ? lo : (hi > n_total ? n_total : hi);
    const int n = hi - lo > max_frames ? max_frames : (int)(hi - lo);
    const float* clip = raw + (size_t)lo * PP_COLS;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int f0 = 0; f0 < n; f0 += PPB_THREADS) {
        const int f = f0 + tid;
        const int keep = f < n && ((f & 1) == 0 || pp_hand_present(clip + (size_t)f * PP_COLS)) ? 1 : 0;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcnt[wid] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wid; ++w) off += s_wcnt[w];
        if (keep) sh[off + before] = f;
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < PPB_THREADS / WAVE; ++w) t += s_wcnt[w]; s_base += t; }
        __syncthreads();
    }
    const int m = s_base;
    const float ratio = m > 0 ? (float)m / (float)Tn : 1.f;
    float* o = out + (size_t)b * Tn * PP_COLS;
    const int nq = Tn * (PP_COLS / 4);
    for (int q = blockIdx.x * PPB_THREADS + tid; q < nq; q += gridDim.x * PPB_THREADS) {
        const int t = q / (PP_COLS / 4), c = (q - t * (PP_COLS / 4)) * 4;
        float4 v;
        v.x = pp_value(clip, sh, n, m, Tn, ratio, t, c + 0, mean, stdv);
        v.y = pp_value(clip, sh, n, m, Tn, ratio, t, c + 1, mean, stdv);
        v.z = pp_value(clip, sh, n, m, Tn, ratio, t, c + 2, mean, stdv);
        v.w = pp_value(clip, sh, n, m, Tn, ratio, t, c + 3, mean, stdv);
        *reinterpret_cast<float4*>(o + (size_t)t * PP_COLS + c) = v;
    }
}

int launch_preprocess_batch(const float* raw, int64_t n_total, const int64_t* offsets, int B, int max_frames, const float* mean, const float* stdv,
                            float* out, int T, hipStream_t s) {
    if (B == 0) return 0;
    // about 1024 workgroups in all (4 per CU) once B >= 64; at most 16 per clip (T = 384: 26 float4 stores per thread at k = 4)
    int k = 1024 / B;
    k = k < 1 ? 1 : (k > 16 ? 16 : k);
    hipLaunchKernelGGL(preprocess_batch_kernel, dim3(k, B), dim3(PPB_THREADS), (size_t)max_frames * sizeof(int), s, raw, n_total, offsets, max_frames,
                       mean, stdv, out, T);
    return launch_rc();
}
