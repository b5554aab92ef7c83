// Training input batch on the device: ASLDataset.__getitem__ (data_loader.py:124-188) + collate for B clips in ONE kernel.
// The raw clips live in a device store [N_frames,124,3] f32; the host draws each clip's augmentation parameters (stretch, shift,
// mirror, finger-dropout windows: ishara_amd/data.py draw_augmentation, the reference's `random` call order) into an
// ishara_clip_aug table, and the kernel maps every output frame to its raw frame through that table:
//   augmented frame j of output frame t: resample down (L2 > T: floor(t * ((L2-1)/(T-1))), the last frame pinned) or pad (t < L2);
//   shifted frame k = j + shift, zero outside [0, L1);  raw frame = floor(k * ((n-1)/(L1-1))) (the last frame pinned);
//   mirror = _HAND_SWAP + negated x;  finger dropout zeroes landmarks 76+f, 97+f where t0 <= j < t1.
// Each index is computed as np.linspace(...).astype(int64) computes it: one fp64 division, one multiply, truncation.
// Then z-normalisation per clip and coordinate over all T*124 values (padded zeros included), two passes in fp64 like numpy
// (mean, then the mean of squared deviations), out = (v - mu) / (sd + 1e-8) in fp64 rounded to f32.
//
// One workgroup (1024 threads) per clip.  A thread owns one 16-byte column chunk of a frame and walks frames slot, slot+nslots, ...,
// so its element -> (landmark, coordinate) map is fixed and computed once: the statistics passes read raw frames as float4 along
// the landmark axis (93 chunks per 1488-byte frame, 11 frames per sweep); the write pass gathers the F output columns (4 per thread,
// F/4 chunks per frame) and stores float4.  Pass 1 streams the clip from HBM; passes 2 and 3 re-read it from L2 / the Infinity Cache.
// Sums are per thread in a fixed frame order, then reduced by a fixed shuffle tree and the 16 wave partials in wave order: no
// atomics, bit-identical from run to run.
#include "kernels.h"

#define CB_THREADS 1024
#define CB_LM 124
#define CB_ROW (CB_LM * 3)               // floats per frame
#define CB_CHUNKS (CB_ROW / 4)           // 93 float4 per frame
#define CB_LEFT 76                       // left hand 76..96, right hand 97..117
#define CB_HAND 21

__device__ __forceinline__ int cb_swap(int l) {   // _HAND_SWAP
    return (l >= CB_LEFT && l < CB_LEFT + CB_HAND) ? l + CB_HAND : ((l >= CB_LEFT + CB_HAND && l < CB_LEFT + 2 * CB_HAND) ? l - CB_HAND : l);
}
// finger index of a hand landmark (dropout bit), -1 elsewhere
__device__ __forceinline__ int cb_finger(int l) {
    return (l >= CB_LEFT && l < CB_LEFT + 2 * CB_HAND) ? (l - CB_LEFT) % CB_HAND : -1;
}
// floor(i * ((p - 1) / (q - 1))) in fp64: np.linspace(0, p-1, q)[i].astype(int64) for i < q-1
__device__ __forceinline__ int cb_lin(int i, int p, int q) {
    const double step = (double)(p - 1) / (double)(q - 1);
    return (int)((double)i * step);
}

__device__ __forceinline__ double cb_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, WAVE);
    return v;
}
// fixed-order block sum of three values; every thread gets the result
__device__ __forceinline__ void cb_block_sum3(double& a, double& b, double& c, double (*red)[3]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    a = cb_wave_sum(a); b = cb_wave_sum(b); c = cb_wave_sum(c);
    if (lane == 0) { red[wid][0] = a; red[wid][1] = b; red[wid][2] = c; }
    __syncthreads();
    a = 0.0; b = 0.0; c = 0.0;
    for (int w = 0; w < CB_THREADS / WAVE; ++w) { a += red[w][0]; b += red[w][1]; c += red[w][2]; }
    __syncthreads();
}

__global__ __launch_bounds__(CB_THREADS) void clip_batch_kernel(const float* __restrict__ raw, const ishara_clip_aug* __restrict__ clips,
                                                                int T, int layout, float* __restrict__ x) {
    __shared__ int s_src[CLIP_MAX_T];   // raw frame (relative to the clip) of output frame t, -1: zero frame
    __shared__ int s_drop[CLIP_MAX_T];  // finger mask active at output frame t
    __shared__ double s_red[CB_THREADS / WAVE][3];
    const int tid = threadIdx.x;
    const ishara_clip_aug a = clips[blockIdx.x];
    const int n = a.n, L1 = a.L1, L2 = a.L2;

    // ---- output frame -> raw frame and dropout mask
    for (int t = tid; t < T; t += CB_THREADS) {
        int src = -1, drop = 0;
        int j = -1;
        if (L2 > T) j = T == 1 ? 0 : (t == T - 1 ? L2 - 1 : cb_lin(t, L2, T));   // linspace(0, L2-1, 1) = [0]
        else if (t < L2) j = t;
        if (j >= 0) {
            const int k = j + a.shift;
            if (k >= 0 && k < L1 && n > 0) {
                src = (L1 == 1) ? 0 : (k == L1 - 1 ? n - 1 : cb_lin(k, n, L1));
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

    const float* clip = raw + (size_t)a.offset * CB_ROW;
    const double sgn_x = a.mirror ? -1.0 : 1.0;
    // statistics mapping: raw chunk q of frames slot, slot + 11, ...; element e of the chunk is raw position 4q+e.  The dropout set
    // {76+f, 97+f} is closed under the hand swap and a sum over all landmarks does not see the permutation, so the statistics read
    // the raw positions directly (x negated when mirrored).
    const int nslots = CB_THREADS / CB_CHUNKS;                   // 11
    const int q = tid % CB_CHUNKS, slot = tid / CB_CHUNKS;
    const bool active = slot < nslots;
    int ec[4], ef[4];                                            // coordinate, finger bit (-1: none) per element
    double es[4];                                                // sign per element
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int p = 4 * q + e;
        ec[e] = p % 3;
        ef[e] = cb_finger(p / 3);
        es[e] = ec[e] == 0 ? sgn_x : 1.0;
    }
    auto value = [&](const float4& v4, int drop, int e) -> double {
        const float f = e == 0 ? v4.x : (e == 1 ? v4.y : (e == 2 ? v4.z : v4.w));
        const bool dropped = ef[e] >= 0 && ((drop >> ef[e]) & 1);
        return dropped ? 0.0 : es[e] * (double)f;
    };
    auto load = [&](int t, int& drop) -> float4 {
        const int src = s_src[t];
        drop = s_drop[t];
        if (src < 0) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *reinterpret_cast<const float4*>(clip + (size_t)src * CB_ROW + 4 * q);
    };

    // ---- pass 1: sums -> mean
    double u[4] = {0.0, 0.0, 0.0, 0.0};                          // per element of the chunk
    if (active) {
        int t = slot;
        for (; t + 3 * nslots < T; t += 4 * nslots) {
            int d0, d1, d2, d3;
            const float4 v0 = load(t, d0), v1 = load(t + nslots, d1), v2 = load(t + 2 * nslots, d2), v3 = load(t + 3 * nslots, d3);
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] += value(v0, d0, e) + value(v1, d1, e) + value(v2, d2, e) + value(v3, d3, e);
        }
        for (; t < T; t += nslots) {
            int d0;
            const float4 v0 = load(t, d0);
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] += value(v0, d0, e);
        }
    }
    // element e has coordinate (q + e) % 3: fold the four element sums onto x, y, z
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { s0 += ec[e] == 0 ? u[e] : 0.0; s1 += ec[e] == 1 ? u[e] : 0.0; s2 += ec[e] == 2 ? u[e] : 0.0; }
    cb_block_sum3(s0, s1, s2, s_red);
    const double cnt = (double)T * (double)CB_LM;
    const double mu0 = s0 / cnt, mu1 = s1 / cnt, mu2 = s2 / cnt;
    double emu[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) emu[e] = ec[e] == 0 ? mu0 : (ec[e] == 1 ? mu1 : mu2);

    // ---- pass 2: squared deviations -> std
#pragma unroll
    for (int e = 0; e < 4; ++e) u[e] = 0.0;
    if (active) {
        int t = slot;
        for (; t + 3 * nslots < T; t += 4 * nslots) {
            int d0, d1, d2, d3;
            const float4 v0 = load(t, d0), v1 = load(t + nslots, d1), v2 = load(t + 2 * nslots, d2), v3 = load(t + 3 * nslots, d3);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double a0 = value(v0, d0, e) - emu[e], a1 = value(v1, d1, e) - emu[e];
                const double a2 = value(v2, d2, e) - emu[e], a3 = value(v3, d3, e) - emu[e];
                u[e] += a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3;
            }
        }
        for (; t < T; t += nslots) {
            int d0;
            const float4 v0 = load(t, d0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double a0 = value(v0, d0, e) - emu[e]; u[e] += a0 * a0; }
        }
    }
    s0 = 0.0; s1 = 0.0; s2 = 0.0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { s0 += ec[e] == 0 ? u[e] : 0.0; s1 += ec[e] == 1 ? u[e] : 0.0; s2 += ec[e] == 2 ? u[e] : 0.0; }
    cb_block_sum3(s0, s1, s2, s_red);
    const double den0 = sqrt(s0 / cnt) + 1e-8, den1 = sqrt(s1 / cnt) + 1e-8, den2 = sqrt(s2 / cnt) + 1e-8;

    // ---- pass 3: gather the output columns, normalise, store.  Output column k of a frame: FLAT k = 3*l + c; HANDS_LIPS_XY
    // k = 2*i + c over the landmarks 76..117, 0..69.  Raw landmark = swap(l) when mirrored; dropout by the output landmark.
    const int F = layout == ISHARA_LAYOUT_FLAT ? CB_ROW : 224;
    const int oq = F / 4, oslots = CB_THREADS / oq;
    const int cq = tid % oq, oslot = tid / oq;
    if (oslot >= oslots) return;
    int rp[4], of[4];                                            // raw position, output finger bit
    double om[4], od[4], osg[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = 4 * cq + e;
        int l, c;
        if (layout == ISHARA_LAYOUT_FLAT) { l = k / 3; c = k % 3; }
        else { const int i = k >> 1; l = i < 2 * CB_HAND ? CB_LEFT + i : i - 2 * CB_HAND; c = k & 1; }
        rp[e] = 3 * (a.mirror ? cb_swap(l) : l) + c;
        of[e] = cb_finger(l);
        om[e] = c == 0 ? mu0 : (c == 1 ? mu1 : mu2);
        od[e] = c == 0 ? den0 : (c == 1 ? den1 : den2);
        osg[e] = c == 0 ? sgn_x : 1.0;
    }
    float* xb = x + (size_t)blockIdx.x * T * F + 4 * cq;
    for (int t = oslot; t < T; t += oslots) {
        const int src = s_src[t], drop = s_drop[t];
        float f[4] = {0.f, 0.f, 0.f, 0.f};
        if (src >= 0) {                                          // a zero frame reads nothing (an empty clip has no frame 0)
            const float* row = clip + (size_t)src * CB_ROW;
#pragma unroll
            for (int e = 0; e < 4; ++e) f[e] = row[rp[e]];
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

int launch_clip_batch(const float* raw, const ishara_clip_aug* clips, int B, int T, int layout, float* x, hipStream_t s) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(clip_batch_kernel, dim3(B), dim3(CB_THREADS), 0, s, raw, clips, T, layout, x);
    return launch_rc();
}
