// What every preprocessing kernel shares (preprocess.hip: one clip, packed ragged clips; stream.hip: fixed-stride session buffers): the part
// tables, the value of one output element and the frame filter's hand-present test.  Included, never copied: a clip's [T,276] is
// bit-identical whichever kernel wrote it because every element goes through the same pp_value.
#pragma once
#include "kernels.h"

#define PP_LM 92
#define PP_COLS 276

// part table (concat order c3:111: lip, rhand, lhand, rpose, lpose): first landmark in the output, offset inside an
// axis block of SEL_COLS (c1:22-26: right hand, left hand, LPOSE, RPOSE, lips)
static __device__ __constant__ int pp_out0[5] = {0, 40, 61, 82, 87};
static __device__ __constant__ int pp_src0[5] = {52, 0, 21, 47, 42};

// Output element (t, c) of one clip: n raw frames, sh[0..m) the kept frames' indices in order, ratio = m / Tn (1 when m == 0).
// Shared by preprocess_kernel, preprocess_batch_kernel and preprocess_sessions_kernel, so that all compute every element with the same operations.
__device__ __forceinline__ float pp_value(const float* __restrict__ raw, const int* sh, int n, int m, int Tn, float ratio, int t, int c,
                                          const float* __restrict__ mean, const float* __restrict__ stdv) {
    const int lm = c / 3, axis = c - lm * 3;
    int part = 0;
#pragma unroll
    for (int p = 1; p < 5; ++p) if (lm >= pp_out0[p]) part = p;
    const int col = axis * PP_LM + pp_src0[part] + (lm - pp_out0[part]);
    float v;
    if (n == 0) v = t == 0 ? 0.f : __builtin_nanf("");     // empty clip -> ONE all-zero frame, NaN padded (c13:11, c3:3-4)
    else if (m < Tn) v = t < m ? raw[(size_t)sh[t] * PP_COLS + col] : __builtin_nanf("");       // NaN pad (c3:3-4)
    else {                                                 // tf.image.resize bilinear, half-pixel centres (c3:6)
        float src = ((float)t + 0.5f) * ratio - 0.5f;
        src = src < 0.f ? 0.f : src;
        int i0 = (int)floorf(src); i0 = i0 > m - 1 ? m - 1 : i0;
        const int i1 = i0 + 1 > m - 1 ? m - 1 : i0 + 1;
        const float w = src - (float)i0;
        v = raw[(size_t)sh[i0] * PP_COLS + col] * (1.f - w) + raw[(size_t)sh[i1] * PP_COLS + col] * w;
    }
    v = (v - mean[c]) / stdv[c];
    return (v != v) ? 0.f : v;                             // NaN -> 0 (c3:114)
}

// hand-present test of one frame (c3:89-93): the sum in preprocess_kernel's order (axis, then landmark), read as float4 / float2
// (a frame row is 1104 bytes and an axis block starts 368 bytes into it: both multiples of 16)
__device__ __forceinline__ bool pp_hand_present(const float* __restrict__ row) {
    float sacc = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float4* p = reinterpret_cast<const float4*>(row + a * PP_LM);
#pragma unroll
        for (int q = 0; q < 10; ++q) {
            const float4 v = p[q];
            sacc += (v.x != v.x) ? 0.f : v.x; sacc += (v.y != v.y) ? 0.f : v.y;
            sacc += (v.z != v.z) ? 0.f : v.z; sacc += (v.w != v.w) ? 0.f : v.w;
        }
        const float2 v = *reinterpret_cast<const float2*>(row + a * PP_LM + 40);
        sacc += (v.x != v.x) ? 0.f : v.x; sacc += (v.y != v.y) ? 0.f : v.y;
    }
    return sacc != 0.f;
}
