// Per-clip frame lengths of the Keras hybrid family ("Frame lengths"): clip b has n_b = frame_len[b] real frames, the frames
// t >= n_b are padding.  Kernels of their own beside the unmasked ones in bn_gate.hip, which stay as they are: the masked time mean that
// feeds the ECA and Squeeze-Excite gates, the two backward passes that hand a gate's gradient to the valid frames only, and the kernel
// that reads the lengths off a zero-padded batch.  frame_len is a device int32 [B], clamped to [0, T] here, never read by the host.
// Activations are [B*T, C] row-major, 16-byte chunks per lane, fp32 arithmetic (as bn_gate.hip).
#include "kernels.h"

DEVI float frame_inv(int n) { return n > 0 ? 1.f / (float)n : 0.f; }      // n_b = 0: both masked means are 0 (Keras: NaN)

// =====================================================================================
// out[b,c] = (sum_{t < n_b} x[b,t,c]) / n_b.  sample_reduce_kernel's layout: grid = (B, ceil(C / 128)), a workgroup owns 128 channels of
// one sample (16 chunk lanes x 16 row lanes, four rows in flight) and writes its means.  Rows at or past n_b are not read.
// =====================================================================================
template <typename T>
__global__ __launch_bounds__(256) void masked_time_mean_kernel(const T* __restrict__ x, const int* __restrict__ frame_len, float* __restrict__ out, int Tn, int C) {
    __shared__ float red[16][16][8];
    const int tid = threadIdx.x, cl = tid & 15, rl = tid >> 4;
    const int b = blockIdx.x;
    const int n = attn_key_count(frame_len, b, Tn);
    const int chunk = blockIdx.y * 16 + cl;
    const bool act = chunk * 8 < C;
    float a[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = 0.f;
    if (act) {
        for (int t0 = rl; t0 < n; t0 += 64) {
            float d[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) load8(x + ((size_t)b * Tn + min(t0 + 16 * u, n - 1)) * C + chunk * 8, d[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t0 + 16 * u < n) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) a[e] += d[u][e];
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rl][cl][e] = a[e];
    __syncthreads();
    if (tid < 128) {            // thread -> channel tid of the 128
        const int c = blockIdx.y * 128 + tid;
        if (c < C) {
            float sa = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) sa += red[r][tid >> 3][tid & 7];
            out[(size_t)b * C + c] = sa * frame_inv(n);
        }
    }
}

int launch_masked_time_mean(int dt, const void* x, const int* frame_len, float* out, int B, int T, int C, hipStream_t s) {
    if (C % 8 != 0) { ishara_set_error("masked_time_mean: C%%8 != 0"); return -1; }
    if (dt == DT_F16) { ishara_set_error("masked_time_mean: ISHARA_F16 has no frame lengths"); return -1; }
    dim3 grid(B, (C + 127) / 128);
    if (dt == DT_BF16) hipLaunchKernelGGL(masked_time_mean_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)x, frame_len, out, T, C);
    else hipLaunchKernelGGL(masked_time_mean_kernel<float>, grid, dim3(256), 0, s, (const float*)x, frame_len, out, T, C);
    return launch_rc();
}

// =====================================================================================
// ECA gate on [B, C] with frame lengths (one workgroup per sample; eca_fwd_kernel's plain form): the pooled value is the mean of BN(h2) over
// the valid frames, g = a[c] * mean[b,c] + bsh[c] with `mean` the masked time mean of h2 — and g = 0 at n_b = 0, where there is nothing to
// pool (not bsh: the mean of no frames is 0, not BN(0)).  s = sigmoid(conv5(g)); P = a*s; Q = bsh*s; the drop-path draw as in eca_fwd_kernel.
// =====================================================================================
__global__ __launch_bounds__(256) void eca_fwd_len_kernel(const float* __restrict__ mean, const float* __restrict__ a, const float* __restrict__ bsh,
                                                          const float* __restrict__ w5, const int* __restrict__ frame_len, int Tn, float* __restrict__ gn,
                                                          float* __restrict__ sg, float* __restrict__ P, float* __restrict__ Q, int C, float* __restrict__ rs, DropSpec dp, int dp_fold) {
    extern __shared__ float sh[];   // [C + 4]
    const int b = blockIdx.x;
    const bool any = attn_key_count(frame_len, b, Tn) > 0;
    for (int c = threadIdx.x; c < C + 4; c += blockDim.x) {
        const int cc = c - 2;
        float g = 0.f;
        if (cc >= 0 && cc < C) {
            g = any ? a[cc] * mean[(size_t)b * C + cc] + bsh[cc] : 0.f;
            gn[(size_t)b * C + cc] = g;
        }
        sh[c] = g;
    }
    __syncthreads();
    const float w0 = w5[0], w1 = w5[1], w2 = w5[2], w3 = w5[3], w4 = w5[4];
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float z = w0 * sh[c] + w1 * sh[c + 1] + w2 * sh[c + 2] + w3 * sh[c + 3] + w4 * sh[c + 4];
        const float sv = sigmoidf_(z);
        sg[(size_t)b * C + c] = sv;
        float r = 1.f;
        if (rs) {
            r = (dp.thr == 0u || rng_keep(rng_row_key(dp.key, (uint32_t)b), 0u, dp.thr)) ? dp.scale : 0.f;
            if (c == 0) rs[b] = r;
            if (!dp_fold) r = 1.f;
        }
        P[(size_t)b * C + c] = a[c] * sv * r;
        Q[(size_t)b * C + c] = bsh[c] * sv * r;
    }
}
int launch_eca_fwd_len(const float* mean, const float* a, const float* b, const float* w5, const int* frame_len, int T,
                       float* gn, float* sgate, float* P, float* Q, int B, int C, hipStream_t s, float* rs, DropSpec dp, int dp_fold) {
    hipLaunchKernelGGL(eca_fwd_len_kernel, dim3(B), dim3(256), (C + 4) * sizeof(float), s, mean, a, b, w5, frame_len, T, gn, sgate, P, Q, C, rs, dp, dp_fold);
    return launch_rc();
}

// =====================================================================================
// Length-gated applies (grid and thread layout of affine_kernel / bn_bwd_apply_kernel: (row blocks, samples), one 8-channel chunk per thread)
// =====================================================================================
// BatchNorm backward of a Conv1DBlock whose ECA gate pooled over the valid frames: dx = a[c] * (dy*sg[b,c] + [t < n_b] Ev[b,c] + Ecol[c] - xhat*Fc[c]).
// Ev[b,c] = dgn[b,c] / n_b is the gate's gradient (valid frames only), Ecol[c] = -dbeta[c] / (B*T) the batch-mean term (every frame).
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_len_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, const float* __restrict__ a, const float* __restrict__ sg,
                                                               const float* __restrict__ Ev, const float* __restrict__ Ecol, const float* __restrict__ Fc,
                                                               const int* __restrict__ frame_len, T* __restrict__ dx, int Tn, int C) {
    const int nch = C >> 3;
    const int cpr = min(nch, 256), rpb = 256 / cpr;
    const int cl = threadIdx.x % cpr, rl = threadIdx.x / cpr;
    const int b = blockIdx.y;
    if (rl >= rpb) return;
    const int n = attn_key_count(frame_len, b, Tn);
    for (int chunk = cl; chunk < nch; chunk += cpr) {
        const int ch = chunk * 8;
        float k0[8], k1[8], k2[8], kv[8];
        {
            float mu[8], rs[8], aa[8], fc[8], ee[8], ec[8], g[8];
            load8(mean + ch, mu); load8(rstd + ch, rs); load8(a + ch, aa); load8(Fc + ch, fc);
            load8(Ev + (size_t)b * C + ch, ee); load8(Ecol + ch, ec); load8(sg + (size_t)b * C + ch, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                k2[e] = aa[e] * rs[e] * fc[e];
                k1[e] = aa[e] * g[e];
                k0[e] = aa[e] * ec[e] + mu[e] * k2[e];
                kv[e] = aa[e] * ee[e];
            }
        }
        for (int t = blockIdx.x * rpb + rl; t < Tn; t += gridDim.x * rpb) {
            const size_t off = ((size_t)b * Tn + t) * C + ch;
            const float gate = t < n ? 1.f : 0.f;
            float d[8], xv[8];
            load8(dy + off, d);
            load8(x + off, xv);
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = d[e] * k1[e] + k0[e] - xv[e] * k2[e] + gate * kv[e];
            store8(dx + off, d);
        }
    }
}

// y = x * P[b,c] + [t < n_b] Q[b,c] / n_b: the Squeeze-Excite backward, du3 = g * se + dz / n_b on the valid frames (dz: the gradient of the masked mean)
template <typename T>
__global__ __launch_bounds__(256) void sample_affine_len_kernel(const T* __restrict__ x, const float* __restrict__ P, const float* __restrict__ Q,
                                                                const int* __restrict__ frame_len, T* __restrict__ y, int Tn, int C) {
    const int nch = C >> 3;
    const int cpr = min(nch, 256), rpb = 256 / cpr;
    const int cl = threadIdx.x % cpr, rl = threadIdx.x / cpr;
    const int b = blockIdx.y;
    if (rl >= rpb) return;
    const int n = attn_key_count(frame_len, b, Tn);
    const float inv = frame_inv(n);
    for (int chunk = cl; chunk < nch; chunk += cpr) {
        float p[8], q[8];
        load8(P + (size_t)b * C + chunk * 8, p);
        load8(Q + (size_t)b * C + chunk * 8, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) q[e] *= inv;
        for (int t = blockIdx.x * rpb + rl; t < Tn; t += gridDim.x * rpb) {
            const size_t off = ((size_t)b * Tn + t) * C + chunk * 8;
            const float gate = t < n ? 1.f : 0.f;
            float v[8];
            load8(x + off, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] * p[e] + gate * q[e];
            store8(y + off, v);
        }
    }
}

static dim3 apply_grid(int B, int T, int C) {
    const int cpr = min(C / 8, 256), rpb = 256 / cpr;
    int gx = (T + rpb - 1) / rpb;
    const int cap = max(1, 4096 / max(B, 1));
    if (gx > cap) gx = cap;
    return dim3(gx, B);
}
int launch_bn_bwd_apply_len(int dt, const void* dy, const void* x, const float* mean, const float* rstd, const float* a, const float* sg,
                            const float* Ev, const float* Ecol, const float* Fc, const int* frame_len, void* dx, int B, int T, int C, hipStream_t s) {
    if (C % 8 != 0 || dt == DT_F16) { ishara_set_error("bn_bwd_apply_len: C%%8 != 0 or ISHARA_F16"); return -1; }
    const dim3 grid = apply_grid(B, T, C);
    if (dt == DT_BF16) hipLaunchKernelGGL(bn_bwd_apply_len_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)dy, (const bf16*)x, mean, rstd, a, sg, Ev, Ecol, Fc, frame_len, (bf16*)dx, T, C);
    else hipLaunchKernelGGL(bn_bwd_apply_len_kernel<float>, grid, dim3(256), 0, s, (const float*)dy, (const float*)x, mean, rstd, a, sg, Ev, Ecol, Fc, frame_len, (float*)dx, T, C);
    return launch_rc();
}
int launch_sample_affine_len(int dt, const void* x, const float* P, const float* Q, const int* frame_len, void* y, int B, int T, int C, hipStream_t s) {
    if (C % 8 != 0 || dt == DT_F16) { ishara_set_error("sample_affine_len: C%%8 != 0 or ISHARA_F16"); return -1; }
    const dim3 grid = apply_grid(B, T, C);
    if (dt == DT_BF16) hipLaunchKernelGGL(sample_affine_len_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)x, P, Q, frame_len, (bf16*)y, T, C);
    else hipLaunchKernelGGL(sample_affine_len_kernel<float>, grid, dim3(256), 0, s, (const float*)x, P, Q, frame_len, (float*)y, T, C);
    return launch_rc();
}

// =====================================================================================
// out_len[b] = 1 + the index of the last frame of clip b with any non-zero feature, 0 if there is none: the prefix reading of Masking(0.0)
// (an all-zero frame inside a clip stays valid).  One workgroup per clip; wave w walks the frames T-1-w, T-5-w, ... and stops at its first
// non-zero one (lanes over the features, a NaN counts as non-zero, -0.0 as zero); the four waves' answers meet in LDS.
// =====================================================================================
__global__ __launch_bounds__(256) void frame_lengths_kernel(const float* __restrict__ x, int Tn, int F, int* __restrict__ out_len) {
    __shared__ int last[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int found = 0;
    for (int t = Tn - 1 - w; t >= 0 && !found; t -= 4) {
        const float* row = x + ((size_t)b * Tn + t) * F;
        int nz = 0;
        for (int f = lane; f < F; f += 64) nz |= (row[f] != 0.f) ? 1 : 0;
        if (__any(nz)) found = t + 1;
    }
    if (lane == 0) last[w] = found;
    __syncthreads();
    if (threadIdx.x == 0) out_len[b] = max(max(last[0], last[1]), max(last[2], last[3]));
}
int launch_frame_lengths(const float* x, int B, int T, int F, int* out_len, hipStream_t s) {
    hipLaunchKernelGGL(frame_lengths_kernel, dim3(B), dim3(256), 0, s, x, T, F, out_len);
    return launch_rc();
}
extern "C" int ishara_frame_lengths(const float* x, int32_t B, int32_t T, int32_t F, int32_t* out_len, ishara_stream st) {
    if (!x || !out_len) { ishara_set_error("ishara_frame_lengths: null x / out_len"); return -1; }
    if (B <= 0 || T <= 0 || F <= 0) { ishara_set_error("ishara_frame_lengths: B, T, F must be positive (got %d, %d, %d)", B, T, F); return -1; }
    if (((uintptr_t)x | (uintptr_t)out_len) % 4 != 0) { ishara_set_error("ishara_frame_lengths: x / out_len must be 4-byte aligned"); return -1; }
    return launch_frame_lengths(x, B, T, F, out_len, (hipStream_t)st);
}
