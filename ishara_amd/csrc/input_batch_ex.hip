// Training input batch with the two augmentations of the reference's CTC training script on top of input_batch.hip's four:
// spatial_random_affine (scale, shear, rotation and one scalar shift of x and y) and temporal_mask (a run of frames blanked), and the
// per-clip frame count written beside x.  The plan is clip_batch_kernel's (input_batch.hip): one workgroup per clip, the output frame ->
// raw frame map and the dropout mask in LDS, two-pass fp64 statistics in a fixed order, one gather-and-store pass with float4 stores.
//   affine: on the raw clip, before the other augmentations, row-vector convention [x' y'] = [x y] * M + shift:
//     x' = f32(f64(M00) x + f64(M10) y + f64(shift)),  y' = f32(f64(M01) x + f64(M11) y + f64(shift)),  z untouched.
//     The two products of f32 values are exact in fp64, so (p + q) is rounded once with or without FMA contraction, then + shift once
//     more: numpy (ishara_amd/data.py affine_xy) and this kernel produce the same bits.  A zero frame (padding, shifted out, masked) and a
//     dropped finger landmark stay exactly 0: the shift is not added to them.  The mirror negates x'.
//   temporal mask: augmented frames m0 <= j < m1 (the index space of the dropout windows) are zero frames: src = -1 in the frame map.
//   frame_len[b] = min(L2, T), 0 for an empty clip; written by thread 0 of the clip's workgroup.
// The statistics are taken over the transformed, f32-rounded values, so x and y of a landmark are needed together: a thread owns three
// consecutive float4 of a frame (12 floats = 4 whole landmarks, 31 groups per 1488-byte frame, 33 frames per sweep) and keeps 16-byte
// loads.  The store pass's HANDS_LIPS_XY chunks are whole (x, y) pairs; FLAT chunks straddle landmarks and load the partner coordinate
// (a cache hit: the neighbouring thread loads the same line).  Sums are per thread in a fixed frame order, then a fixed shuffle tree
// and the 16 wave partials in wave order: no atomics, bit-identical from run to run.
#include "kernels.h"

static_assert(sizeof(ishara_clip_aug_ex) == 96, "ishara_clip_aug_ex is 96 bytes");

#define CX_THREADS 1024
#define CX_LM 124
#define CX_ROW (CX_LM * 3)               // floats per frame
#define CX_GROUPS (CX_LM / 4)            // 31 groups of 4 landmarks (3 float4) per frame
#define CX_LEFT 76                       // left hand 76..96, right hand 97..117
#define CX_HAND 21

__device__ __forceinline__ int cx_swap(int l) {   // _HAND_SWAP
    return (l >= CX_LEFT && l < CX_LEFT + CX_HAND) ? l + CX_HAND : ((l >= CX_LEFT + CX_HAND && l < CX_LEFT + 2 * CX_HAND) ? l - CX_HAND : l);
}
// finger index of a hand landmark (dropout bit), -1 elsewhere
__device__ __forceinline__ int cx_finger(int l) {
    return (l >= CX_LEFT && l < CX_LEFT + 2 * CX_HAND) ? (l - CX_LEFT) % CX_HAND : -1;
}
// floor(i * ((p - 1) / (q - 1))) in fp64: np.linspace(0, p-1, q)[i].astype(int64) for i < q-1
__device__ __forceinline__ int cx_lin(int i, int p, int q) {
    const double step = (double)(p - 1) / (double)(q - 1);
    return (int)((double)i * step);
}
// one coordinate of the affine: f32((a u + b v) + s), a, b, u, v f32 values carried in fp64
__device__ __forceinline__ float cx_affine(double a, double b, double s, float u, float v) {
    return (float)((a * (double)u + b * (double)v) + s);
}

__device__ __forceinline__ double cx_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, WAVE);
    return v;
}
// fixed-order block sum of three values; every thread gets the result
__device__ __forceinline__ void cx_block_sum3(double& a, double& b, double& c, double (*red)[3]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    a = cx_wave_sum(a); b = cx_wave_sum(b); c = cx_wave_sum(c);
    if (lane == 0) { red[wid][0] = a; red[wid][1] = b; red[wid][2] = c; }
    __syncthreads();
    a = 0.0; b = 0.0; c = 0.0;
    for (int w = 0; w < CX_THREADS / WAVE; ++w) { a += red[w][0]; b += red[w][1]; c += red[w][2]; }
    __syncthreads();
}

struct cx_group { float4 a, b, c; };     // 4 landmarks: (a.x a.y a.z) (a.w b.x b.y) (b.z b.w c.x) (c.y c.z c.w)

template <int LAYOUT>
__global__ __launch_bounds__(CX_THREADS) void clip_batch_ex_kernel(const float* __restrict__ raw, const ishara_clip_aug_ex* __restrict__ clips,
                                                                   int T, float* __restrict__ x, int* __restrict__ frame_len) {
    __shared__ int s_src[CLIP_MAX_T];   // raw frame (relative to the clip) of output frame t, -1: zero frame
    __shared__ int s_drop[CLIP_MAX_T];  // finger mask active at output frame t
    __shared__ double s_red[CX_THREADS / WAVE][3];
    const int tid = threadIdx.x;
    const ishara_clip_aug_ex ax = clips[blockIdx.x];
    const ishara_clip_aug& a = ax.base;
    const int n = a.n, L1 = a.L1, L2 = a.L2;
    if (tid == 0 && frame_len) frame_len[blockIdx.x] = n > 0 ? max(0, min(L2, T)) : 0;

    // ---- output frame -> raw frame and dropout mask
    for (int t = tid; t < T; t += CX_THREADS) {
        int src = -1, drop = 0;
        int j = -1;
        if (L2 > T) j = T == 1 ? 0 : (t == T - 1 ? L2 - 1 : cx_lin(t, L2, T));   // linspace(0, L2-1, 1) = [0]
        else if (t < L2) j = t;
        if (j >= 0 && !(j >= ax.m0 && j < ax.m1)) {                              // a masked frame is a zero frame
            const int k = j + a.shift;
            if (k >= 0 && k < L1 && n > 0) {
                src = (L1 == 1) ? 0 : (k == L1 - 1 ? n - 1 : cx_lin(k, n, L1));
                src = src < 0 ? 0 : (src > n - 1 ? n - 1 : src);
#pragma unroll
                for (int w = 0; w < 3; ++w)
                    if (j >= a.t0[w] && j < a.t1[w]) drop |= a.fingers[w];
            }
        }
        s_src[t] = src;
        s_drop[t] = drop;
    }
    __syncthreads();

    const float* clip = raw + (size_t)a.offset * CX_ROW;
    const double sgn_x = a.mirror ? -1.0 : 1.0;
    const double m00 = (double)ax.m[0], m01 = (double)ax.m[1], m10 = (double)ax.m[2], m11 = (double)ax.m[3], sh = (double)ax.shift_xy;
    // statistics mapping: landmarks 4g .. 4g+3 of frames slot, slot + 33, ...  The dropout set {76+f, 97+f} is closed under the hand swap
    // and a sum over all landmarks does not see the permutation, so the statistics read the raw positions directly (x' negated when
    // mirrored).
    const int nslots = CX_THREADS / CX_GROUPS;                   // 33
    const int g = tid % CX_GROUPS, slot = tid / CX_GROUPS;
    const bool active = slot < nslots;
    int ef[4];                                                   // finger bit (-1: none) per landmark of the group
#pragma unroll
    for (int i = 0; i < 4; ++i) ef[i] = cx_finger(4 * g + i);
    auto load = [&](int t, int& drop) -> cx_group {              // drop = -1: a zero frame
        const int src = s_src[t];
        drop = s_drop[t];
        cx_group v;
        if (src < 0) { drop = -1; v.a = v.b = v.c = make_float4(0.f, 0.f, 0.f, 0.f); return v; }
        const float4* p = reinterpret_cast<const float4*>(clip + (size_t)src * CX_ROW + 12 * g);
        v.a = p[0]; v.b = p[1]; v.c = p[2];
        return v;
    };
    // the transformed (x', y', z) of the group's 4 landmarks as they enter the statistics: 0 on a zero frame or a dropped landmark
    auto values = [&](const cx_group& v, int drop, double (*o)[3]) {
        const float r[12] = {v.a.x, v.a.y, v.a.z, v.a.w, v.b.x, v.b.y, v.b.z, v.b.w, v.c.x, v.c.y, v.c.z, v.c.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool zero = drop < 0 || (ef[i] >= 0 && ((drop >> ef[i]) & 1));
            o[i][0] = zero ? 0.0 : sgn_x * (double)cx_affine(m00, m10, sh, r[3 * i], r[3 * i + 1]);
            o[i][1] = zero ? 0.0 : (double)cx_affine(m01, m11, sh, r[3 * i], r[3 * i + 1]);
            o[i][2] = zero ? 0.0 : (double)r[3 * i + 2];
        }
    };

    // ---- pass 1: sums -> mean
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    if (active) {
        int t = slot;
        for (; t + nslots < T; t += 2 * nslots) {
            int d0, d1;
            const cx_group v0 = load(t, d0), v1 = load(t + nslots, d1);
            double o0[4][3], o1[4][3];
            values(v0, d0, o0); values(v1, d1, o1);
#pragma unroll
            for (int i = 0; i < 4; ++i) { s0 += o0[i][0] + o1[i][0]; s1 += o0[i][1] + o1[i][1]; s2 += o0[i][2] + o1[i][2]; }
        }
        for (; t < T; t += nslots) {
            int d0;
            const cx_group v0 = load(t, d0);
            double o0[4][3];
            values(v0, d0, o0);
#pragma unroll
            for (int i = 0; i < 4; ++i) { s0 += o0[i][0]; s1 += o0[i][1]; s2 += o0[i][2]; }
        }
    }
    cx_block_sum3(s0, s1, s2, s_red);
    const double cnt = (double)T * (double)CX_LM;
    const double mu0 = s0 / cnt, mu1 = s1 / cnt, mu2 = s2 / cnt;

    // ---- pass 2: squared deviations -> std
    s0 = 0.0; s1 = 0.0; s2 = 0.0;
    if (active) {
        int t = slot;
        for (; t + nslots < T; t += 2 * nslots) {
            int d0, d1;
            const cx_group v0 = load(t, d0), v1 = load(t + nslots, d1);
            double o0[4][3], o1[4][3];
            values(v0, d0, o0); values(v1, d1, o1);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double a0 = o0[i][0] - mu0, a1 = o0[i][1] - mu1, a2 = o0[i][2] - mu2;
                const double b0 = o1[i][0] - mu0, b1 = o1[i][1] - mu1, b2 = o1[i][2] - mu2;
                s0 += a0 * a0 + b0 * b0; s1 += a1 * a1 + b1 * b1; s2 += a2 * a2 + b2 * b2;
            }
        }
        for (; t < T; t += nslots) {
            int d0;
            const cx_group v0 = load(t, d0);
            double o0[4][3];
            values(v0, d0, o0);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double a0 = o0[i][0] - mu0, a1 = o0[i][1] - mu1, a2 = o0[i][2] - mu2;
                s0 += a0 * a0; s1 += a1 * a1; s2 += a2 * a2;
            }
        }
    }
    cx_block_sum3(s0, s1, s2, s_red);
    const double den0 = sqrt(s0 / cnt) + 1e-8, den1 = sqrt(s1 / cnt) + 1e-8, den2 = sqrt(s2 / cnt) + 1e-8;

    // ---- pass 3: gather the output columns, transform, normalise, store.  Output column k of a frame: FLAT k = 3*l + c; HANDS_LIPS_XY
    // k = 2*i + c over the landmarks 76..117, 0..69.  Raw landmark = swap(l) when mirrored; dropout by the output landmark.
    constexpr int F = LAYOUT == ISHARA_LAYOUT_FLAT ? CX_ROW : 224;
    constexpr int oq = F / 4, oslots = CX_THREADS / oq;
    const int cq = tid % oq, oslot = tid / oq;
    if (oslot >= oslots) return;
    int rb[4], of[4];                                            // raw landmark base (3 * landmark), output finger bit
    bool isz[4];
    double ea[4], eb[4], om[4], od[4], osg[4];                   // x' / y' row of M, mean, denominator, sign per element
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * cq + e;
        int l, c;
        if (LAYOUT == ISHARA_LAYOUT_FLAT) { l = k / 3; c = k % 3; }
        else { const int i = k >> 1; l = i < 2 * CX_HAND ? CX_LEFT + i : i - 2 * CX_HAND; c = k & 1; }
        rb[e] = 3 * (a.mirror ? cx_swap(l) : l);
        of[e] = cx_finger(l);
        isz[e] = c == 2;
        ea[e] = c == 0 ? m00 : m01;
        eb[e] = c == 0 ? m10 : m11;
        om[e] = c == 0 ? mu0 : (c == 1 ? mu1 : mu2);
        od[e] = c == 0 ? den0 : (c == 1 ? den1 : den2);
        osg[e] = c == 0 ? sgn_x : 1.0;
    }
    float* xb = x + (size_t)blockIdx.x * T * F + 4 * cq;
    for (int t = oslot; t < T; t += oslots) {
        const int src = s_src[t], drop = s_drop[t];
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        if (src >= 0) {                                          // a zero frame reads nothing (an empty clip has no frame 0)
            const float* row = clip + (size_t)src * CX_ROW;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float u = row[rb[e] + (isz[e] ? 2 : 0)], v = row[rb[e] + 1];     // z, or x with its partner y
                const float w = cx_affine(ea[e], eb[e], sh, u, v);
                f[e] = isz[e] ? u : w;
            }
        }
        float r[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool zero = src < 0 || (of[e] >= 0 && ((drop >> of[e]) & 1));
            const double v = zero ? 0.0 : osg[e] * (double)f[e];
            r[e] = (float)((v - om[e]) / od[e]);
        }
        *reinterpret_cast<float4*>(xb + (size_t)t * F) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

int launch_clip_batch_ex(const float* raw, const ishara_clip_aug_ex* clips, int B, int T, int layout, float* x, int* frame_len, hipStream_t s) {
    if (B == 0) return 0;
    if (layout == ISHARA_LAYOUT_FLAT)
        hipLaunchKernelGGL(clip_batch_ex_kernel<ISHARA_LAYOUT_FLAT>, dim3(B), dim3(CX_THREADS), 0, s, raw, clips, T, x, frame_len);
    else
        hipLaunchKernelGGL(clip_batch_ex_kernel<ISHARA_LAYOUT_HANDS_LIPS_XY>, dim3(B), dim3(CX_THREADS), 0, s, raw, clips, T, x, frame_len);
    return launch_rc();
}
