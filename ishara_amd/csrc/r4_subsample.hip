// The torch Squeezeformer family's small kernels, everything of the encoder that is neither a GEMM, a norm, the ConvModule nor the attention
// (relattn_len.hip / relattn_mfma.hip): DepthwiseConv2dSubsampling (convolution.py:39-73), TimeReductionLayer (:241-269), the row maps of
// recover_resolution / the crop / the residual wrapper (modules.py:137-142, encoder.py:157-162) and the per-clip length arithmetic of the masked
// pass, forward and backward, one thread per output element (the three *_bwd_w kernels: one workgroup sum per parameter).  Each kernel's launch
// is stated here once, grid included, and shared by the encoder (squeezeformer_r4.hip) and the operator entry points (api_ops.hip ishara_op_r4_*).
#include "model_types.h"

template <typename T> DEVI float ldf(const T* p) { return to_f(*p); }

// the tail of the three *_bwd_w kernels (256 threads): the workgroup's sums of acc[0..9] through LDS, then dw[0..8] += the first nine and
// db[0] += the tenth; ATOMIC where several workgroups add into the same ten words
template <bool ATOMIC>
DEVI void r4_wsum10_add(const float (&acc)[10], float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float red[10][256];
    for (int q = 0; q < 10; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) for (int q = 0; q < 10; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        __syncthreads();
    }
    if (ATOMIC) {
        if (threadIdx.x < 9) atomicAdd(&dw[threadIdx.x], red[threadIdx.x][0]);
        if (threadIdx.x == 9) atomicAdd(&db[0], red[9][0]);
    } else {
        if (threadIdx.x < 9) dw[threadIdx.x] += red[threadIdx.x][0];
        if (threadIdx.x == 9) db[0] += red[9][0];
    }
}

// x [B,T0,F] f32 -> y1 [B,d,T1,F1] f32 = relu(conv3x3 s2)        (convolution.py:56)
__global__ void r4_sub1_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ y1,
                            int B, int T0, int F, int d, int T1, int F1) {
    const size_t n = (size_t)B * d * T1 * F1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int f1 = (int)(i % F1), t1 = (int)((i / F1) % T1), c = (int)((i / ((size_t)F1 * T1)) % d), bb = (int)(i / ((size_t)F1 * T1 * d));
        float acc = b[c];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int e = 0; e < 3; ++e) acc += w[c * 9 + a * 3 + e] * x[((size_t)bb * T0 + 2 * t1 + a) * F + 2 * f1 + e];
        y1[i] = fmaxf(acc, 0.f);
    }
}
// y1 -> sub [B*T2, d*F2] (storage type) = relu(depthwise conv3x3 s2), channel-major features   (:58-66)
template <typename T>
__global__ void r4_sub2_fwd(const float* __restrict__ y1, const float* __restrict__ w, const float* __restrict__ b, T* __restrict__ sub,
                            int B, int d, int T1, int F1, int T2, int F2) {
    const size_t n = (size_t)B * T2 * d * F2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int f2 = (int)(i % F2), c = (int)((i / F2) % d), t2 = (int)((i / ((size_t)F2 * d)) % T2), bb = (int)(i / ((size_t)F2 * d * T2));
        float acc = b[c];
        const float* src = y1 + (((size_t)bb * d + c) * T1) * F1;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int e = 0; e < 3; ++e) acc += w[c * 9 + a * 3 + e] * src[(size_t)(2 * t2 + a) * F1 + 2 * f2 + e];
        sub[i] = from_f<T>(fmaxf(acc, 0.f));
    }
}
// backward of the depthwise conv: dz2 = dsub * (sub > 0); dw2, db2 (atomics) and dy1 (scatter-free gather form)
template <typename T>
__global__ void r4_sub2_bwd_w(const T* __restrict__ dsub, const T* __restrict__ sub, const float* __restrict__ y1, float* __restrict__ dw, float* __restrict__ db,
                              int B, int d, int T1, int F1, int T2, int F2) {
    // one workgroup per channel: 10 sums over (b, t2, f2)
    const int c = blockIdx.x;
    float acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int n = B * T2 * F2;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int f2 = i % F2, t2 = (i / F2) % T2, bb = i / (F2 * T2);
        const size_t o = (((size_t)bb * T2 + t2) * d + c) * F2 + f2;
        const float g = ldf(sub + o) > 0.f ? ldf(dsub + o) : 0.f;
        const float* src = y1 + (((size_t)bb * d + c) * T1) * F1;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[a * 3 + e] += g * src[(size_t)(2 * t2 + a) * F1 + 2 * f2 + e];
        acc[9] += g;
    }
    r4_wsum10_add<false>(acc, dw + c * 9, db + c);
}
template <typename T>
__global__ void r4_sub2_bwd_x(const T* __restrict__ dsub, const T* __restrict__ sub, const float* __restrict__ w, const float* __restrict__ y1, float* __restrict__ dz1,
                              int B, int d, int T1, int F1, int T2, int F2) {
    // dz1[b,c,t1,f1] = (y1 > 0) * sum_{a,e: (t1-a)/2, (f1-e)/2 integral and in range} w[c,a,e] * dz2[b, (t1-a)/2, c, (f1-e)/2]
    const size_t n = (size_t)B * d * T1 * F1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int f1 = (int)(i % F1), t1 = (int)((i / F1) % T1), c = (int)((i / ((size_t)F1 * T1)) % d), bb = (int)(i / ((size_t)F1 * T1 * d));
        float acc = 0.f;
        if (y1[i] > 0.f) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int tt = t1 - a;
                if (tt < 0 || (tt & 1) || (tt >> 1) >= T2) continue;
#pragma unroll
                for (int e = 0; e < 3; ++e) {
                    const int ff = f1 - e;
                    if (ff < 0 || (ff & 1) || (ff >> 1) >= F2) continue;
                    const size_t o = (((size_t)bb * T2 + (tt >> 1)) * d + c) * F2 + (ff >> 1);
                    if (ldf(sub + o) > 0.f) acc += w[c * 9 + a * 3 + e] * ldf(dsub + o);
                }
            }
        }
        dz1[i] = acc;
    }
}
// first conv backward: dw1[c,9], db1[c] from dz1 and x (one workgroup per channel); dx optional (atomic-free gather over channels is O(d): skipped unless asked)
__global__ void r4_sub1_bwd_w(const float* __restrict__ dz1, const float* __restrict__ x, float* __restrict__ dw, float* __restrict__ db,
                              int B, int T0, int F, int d, int T1, int F1) {
    const int c = blockIdx.x;
    float acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int n = B * T1 * F1;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int f1 = i % F1, t1 = (i / F1) % T1, bb = i / (F1 * T1);
        const float g = dz1[(((size_t)bb * d + c) * T1 + t1) * F1 + f1];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[a * 3 + e] += g * x[((size_t)bb * T0 + 2 * t1 + a) * F + 2 * f1 + e];
        acc[9] += g;
    }
    r4_wsum10_add<false>(acc, dw + c * 9, db + c);
}
__global__ void r4_sub1_bwd_x(const float* __restrict__ dz1, const float* __restrict__ w, float* __restrict__ dx, int B, int T0, int F, int d, int T1, int F1) {
    const size_t n = (size_t)B * T0 * F;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % F), t = (int)((i / F) % T0), bb = (int)(i / ((size_t)F * T0));
        float acc = 0.f;
        for (int a = 0; a < 3; ++a) {
            const int tt = t - a;
            if (tt < 0 || (tt & 1) || (tt >> 1) >= T1) continue;
            for (int e = 0; e < 3; ++e) {
                const int ff = f - e;
                if (ff < 0 || (ff & 1) || (ff >> 1) >= F1) continue;
                for (int c = 0; c < d; ++c) acc += w[c * 9 + a * 3 + e] * dz1[(((size_t)bb * d + c) * T1 + (tt >> 1)) * F1 + (ff >> 1)];
            }
        }
        dx[i] = acc;
    }
}

// TimeReductionLayer (convolution.py:241-269): one 3x3 stride-2 kernel over the (time, feature) plane of h [B,Tin,d], Swish;
// out [B*Tr, Kp] (columns >= Fr are zero padding of the following Linear's K), pre [B,Tr,Fr] f32 saved for the backward pass
template <typename T>
__global__ void r4_tred_fwd(const T* __restrict__ h, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ pre, T* __restrict__ out,
                            int B, int Tin, int d, int Tr, int Fr, int Kp) {
    const size_t n = (size_t)B * Tr * Kp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % Kp), t = (int)((i / Kp) % Tr), bb = (int)(i / ((size_t)Kp * Tr));
        if (f >= Fr) { out[i] = from_f<T>(0.f); continue; }
        float acc = b[0];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int e = 0; e < 3; ++e) acc += w[a * 3 + e] * ldf(h + ((size_t)bb * Tin + 2 * t + a) * d + 2 * f + e);
        pre[((size_t)bb * Tr + t) * Fr + f] = acc;
        out[i] = from_f<T>(swishf_(acc));
    }
}
template <typename T>
__global__ void r4_tred_bwd_w(const T* __restrict__ dout, const float* __restrict__ pre, const T* __restrict__ h, float* __restrict__ dw, float* __restrict__ db,
                              int B, int Tin, int d, int Tr, int Fr, int Kp) {
    float acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const size_t n = (size_t)B * Tr * Fr;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % Fr), t = (int)((i / Fr) % Tr), bb = (int)(i / ((size_t)Fr * Tr));
        const float g = ldf(dout + ((size_t)bb * Tr + t) * Kp + f) * dswishf_(pre[i]);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int e = 0; e < 3; ++e) acc[a * 3 + e] += g * ldf(h + ((size_t)bb * Tin + 2 * t + a) * d + 2 * f + e);
        acc[9] += g;
    }
    r4_wsum10_add<true>(acc, dw, db);
}
// dh[b,t,f] = extra[b,t,f] (gradient arriving through the recover skip, or 0) + sum_{a,e} w[a,e] * dz[b, (t-a)/2, (f-e)/2]
template <typename T>
__global__ void r4_tred_bwd_x(const T* __restrict__ dout, const float* __restrict__ pre, const float* __restrict__ w, const T* __restrict__ extra, T* __restrict__ dh,
                              int B, int Tin, int d, int Tr, int Fr, int Kp) {
    const size_t n = (size_t)B * Tin * d;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int f = (int)(i % d), t = (int)((i / d) % Tin), bb = (int)(i / ((size_t)d * Tin));
        float acc = extra ? ldf(extra + i) : 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int tt = t - a;
            if (tt < 0 || (tt & 1) || (tt >> 1) >= Tr) continue;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const int ff = f - e;
                if (ff < 0 || (ff & 1) || (ff >> 1) >= Fr) continue;
                const size_t o = ((size_t)bb * Tr + (tt >> 1));
                acc += w[a * 3 + e] * ldf(dout + o * Kp + (ff >> 1)) * dswishf_(pre[o * Fr + (ff >> 1)]);
            }
        }
        dh[i] = from_f<T>(acc);
    }
}
// generic row maps over [B, Tdst, d], MODE one of R4_ROWS_* (model_types.h; the integers are the ABI of ishara_op_r4_rows):
//   0 RECOVER      dst[b,t] = src[b, t/2] (recover_resolution, src has Tsrc rows per sample)
//   1 CROP         dst[b,t] = src[b,t] for t < Tdst (crop of a longer sequence)
//   2 RECOVER_BWD  dst[b,t] = src[b,2t] + src[b,2t+1] (backward of RECOVER)
//   3 CROP_BWD     dst[b,t] = t < Tsrc ? src[b,t] : 0 (backward of the crop into the longer sequence)
//   4 ADD          dst = a + src (same shape)
template <typename T, int MODE>
__global__ void r4_rows(const T* __restrict__ src, const T* __restrict__ a, T* __restrict__ dst, int B, int Tdst, int Tsrc, int d) {
    const size_t n = (size_t)B * Tdst * d;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int e = (int)(i % d), t = (int)((i / d) % Tdst), bb = (int)(i / ((size_t)d * Tdst));
        float v;
        if (MODE == R4_ROWS_RECOVER) v = ldf(src + ((size_t)bb * Tsrc + (t >> 1)) * d + e);
        else if (MODE == R4_ROWS_CROP) v = ldf(src + ((size_t)bb * Tsrc + t) * d + e);
        else if (MODE == R4_ROWS_RECOVER_BWD) v = ldf(src + ((size_t)bb * Tsrc + 2 * t) * d + e) + ldf(src + ((size_t)bb * Tsrc + 2 * t + 1) * d + e);
        else if (MODE == R4_ROWS_CROP_BWD) v = t < Tsrc ? ldf(src + ((size_t)bb * Tsrc + t) * d + e) : 0.f;
        else v = ldf(a + i) + ldf(src + i);
        dst[i] = from_f<T>(v);
    }
}
__global__ void r4_axpy_f32(const float* __restrict__ x, float* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] += x[i];
}
__global__ void r4_fill_f32(float* p, size_t n, float v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
static int g1d(size_t n) { const size_t g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }
template <int MODE>
static int r4_rows_launch(int dt, const void* src, const void* a, void* dst, int B, int Tdst, int Tsrc, int d, hipStream_t s) {
    const int grid = g1d((size_t)B * Tdst * d);
    if (dt == DT_BF16) hipLaunchKernelGGL((r4_rows<bf16, MODE>), dim3(grid), dim3(256), 0, s, (const bf16*)src, (const bf16*)a, (bf16*)dst, B, Tdst, Tsrc, d);
    else hipLaunchKernelGGL((r4_rows<float, MODE>), dim3(grid), dim3(256), 0, s, (const float*)src, (const float*)a, (float*)dst, B, Tdst, Tsrc, d);
    return launch_rc();
}
int r4_rows_mode_launch(int dt, int mode, const void* src, const void* a, void* dst, int B, int Tdst, int Tsrc, int d, hipStream_t s) {
    switch (mode) {
        case R4_ROWS_RECOVER: return r4_rows_launch<R4_ROWS_RECOVER>(dt, src, a, dst, B, Tdst, Tsrc, d, s);
        case R4_ROWS_CROP: return r4_rows_launch<R4_ROWS_CROP>(dt, src, a, dst, B, Tdst, Tsrc, d, s);
        case R4_ROWS_RECOVER_BWD: return r4_rows_launch<R4_ROWS_RECOVER_BWD>(dt, src, a, dst, B, Tdst, Tsrc, d, s);
        case R4_ROWS_CROP_BWD: return r4_rows_launch<R4_ROWS_CROP_BWD>(dt, src, a, dst, B, Tdst, Tsrc, d, s);
        case R4_ROWS_ADD: return r4_rows_launch<R4_ROWS_ADD>(dt, src, a, dst, B, Tdst, Tsrc, d, s);
        default: ishara_set_error("r4_rows: unknown mode %d (0..4)", mode); return -1;
    }
}

// typed launches of the small kernels
#define R4_TYPED(dt, CALL) do { if ((dt) == DT_BF16) { typedef bf16 TT; CALL; } else { typedef float TT; CALL; } } while (0)

// ---- the launches of the subsampling and time-reduction kernels, shared by the encoder (r4_forward / r4_backward) and the operator entry
// points (api_ops.hip ishara_op_r4_*): grids included
R4Dims r4_dims(int T0, int F, int d) {
    R4Dims D;
    D.T1 = (T0 - 3) / 2 + 1; D.F1 = (F - 3) / 2 + 1;
    D.T2 = (D.T1 - 3) / 2 + 1; D.F2 = (D.F1 - 3) / 2 + 1;
    D.T3 = (D.T2 - 3) / 2 + 1; D.Fr = (d - 1) / 2; D.Kp = (int)rup(D.Fr, 8);
    return D;
}
// x [B,T0,F] f32 -> y1 [B,d,T1,F1] f32 -> sub [B*T2, d*F2] (dt)
int r4_subsample_fwd_launch(int dt, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y1, void* sub,
                            int B, int T0, int F, int d, int T1, int F1, int T2, int F2, hipStream_t s) {
    hipLaunchKernelGGL(r4_sub1_fwd, dim3(g1d((size_t)B * d * T1 * F1)), dim3(256), 0, s, x, w1, b1, y1, B, T0, F, d, T1, F1);
    R4_TYPED(dt, hipLaunchKernelGGL((r4_sub2_fwd<TT>), dim3(g1d((size_t)B * T2 * d * F2)), dim3(256), 0, s, y1, w2, b2, (TT*)sub, B, d, T1, F1, T2, F2));
    return launch_rc();
}
// dsub -> dw2, db2, dz1 (scratch [B,d,T1,F1] f32), dw1, db1 (all four accumulated) and dx (NULL: skipped)
int r4_subsample_bwd_launch(int dt, const void* dsub, const void* sub, const float* y1, const float* x, const float* w1, const float* w2, float* dz1,
                            float* dw1, float* db1, float* dw2, float* db2, float* dx, int B, int T0, int F, int d, int T1, int F1, int T2, int F2, hipStream_t s) {
    R4_TYPED(dt, hipLaunchKernelGGL((r4_sub2_bwd_w<TT>), dim3(d), dim3(256), 0, s, (const TT*)dsub, (const TT*)sub, y1, dw2, db2, B, d, T1, F1, T2, F2));
    R4_TYPED(dt, hipLaunchKernelGGL((r4_sub2_bwd_x<TT>), dim3(g1d((size_t)B * d * T1 * F1)), dim3(256), 0, s, (const TT*)dsub, (const TT*)sub, w2, y1, dz1, B, d, T1, F1, T2, F2));
    hipLaunchKernelGGL(r4_sub1_bwd_w, dim3(d), dim3(256), 0, s, dz1, x, dw1, db1, B, T0, F, d, T1, F1);
    if (dx) hipLaunchKernelGGL(r4_sub1_bwd_x, dim3(g1d((size_t)B * T0 * F)), dim3(256), 0, s, dz1, w1, dx, B, T0, F, d, T1, F1);
    return launch_rc();
}
// h [B,Tin,d] (dt) -> pre [B,Tr,Fr] f32, out [B*Tr, Kp] (dt, pad columns zero)
int r4_tred_fwd_launch(int dt, const void* h, const float* w, const float* b, float* pre, void* out, int B, int Tin, int d, int Tr, int Fr, int Kp, hipStream_t s) {
    R4_TYPED(dt, hipLaunchKernelGGL((r4_tred_fwd<TT>), dim3(g1d((size_t)B * Tr * Kp)), dim3(256), 0, s, (const TT*)h, w, b, pre, (TT*)out, B, Tin, d, Tr, Fr, Kp));
    return launch_rc();
}
// weight gradient of time_reduction_proj over the padded K (the pad columns of trout are zero, so are the rows >= Fr of the product): into the
// [Kp, d] scratch dwred, then the Fr real rows are added to dW; the bias gradient is added to db
int r4_tred_wgrad_launch(int dt, const void* trout, const void* g, float* dwred, float* dW, float* db, float* slab, int M, int Fr, int Kp, int d, hipStream_t s) {
    OpArgs no;
    hipLaunchKernelGGL(r4_fill_f32, dim3(g1d((size_t)Kp * d)), dim3(256), 0, s, dwred, (size_t)Kp * d, 0.f);
    CK(launch_gemm_tn(dt, dt, dt, OP_NONE, OP_NONE, trout, g, dwred, db, slab, M, Kp, d, no, no, s));
    hipLaunchKernelGGL(r4_axpy_f32, dim3(g1d((size_t)Fr * d)), dim3(256), 0, s, dwred, dW, (size_t)Fr * d);
    return launch_rc();
}
// dout [B*Tr, Kp] (dt: gradient of the conv output) -> dw[9], db[1] (accumulated), dh [B,Tin,d] = extra (NULL: 0) + the input gradient
int r4_tred_bwd_launch(int dt, const void* dout, const float* pre, const void* h, const float* w, const void* extra, float* dw, float* db, void* dh,
                       int B, int Tin, int d, int Tr, int Fr, int Kp, hipStream_t s) {
    R4_TYPED(dt, hipLaunchKernelGGL((r4_tred_bwd_w<TT>), dim3(64), dim3(256), 0, s, (const TT*)dout, pre, (const TT*)h, dw, db, B, Tin, d, Tr, Fr, Kp));
    R4_TYPED(dt, hipLaunchKernelGGL((r4_tred_bwd_x<TT>), dim3(g1d((size_t)B * Tin * d)), dim3(256), 0, s, (const TT*)dout, pre, w, (const TT*)extra, (TT*)dh, B, Tin, d, Tr, Fr, Kp));
    return launch_rc();
}
int r4_fill_f32_launch(float* p, size_t n, float v, hipStream_t s) {
    hipLaunchKernelGGL(r4_fill_f32, dim3(g1d(n)), dim3(256), 0, s, p, n, v);
    return launch_rc();
}

// ------------------------------------------------------------------ stage lengths
// input frames L[b] -> keys of each attention resolution, the reference's own arithmetic, clamped, on the device (the host never reads them):
//   n2 = clamp((L >> 2) - 1, 0, T2) (convolution.py:68-71), n3 = clamp((n2 >> 1) - 1, 0, T3) (:266-268), nrec = clamp(2 * n3, 0, Trec) (encoder.py:162)
// out int32 [3][B]
__global__ void r4_stage_len_kernel(const int* __restrict__ L, int* __restrict__ out, int B, int T0, int T2, int T3, int Trec) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int l = min(max(L[b], 0), T0);
    const int n2 = min(max((l >> 2) - 1, 0), T2);
    const int n3 = min(max((n2 >> 1) - 1, 0), T3);
    out[b] = n2; out[B + b] = n3; out[2 * B + b] = min(max(2 * n3, 0), Trec);
}
int r4_stage_len_launch(const int* L, int* out, int B, int T0, int T2, int T3, int Trec, hipStream_t s) {
    hipLaunchKernelGGL(r4_stage_len_kernel, dim3((B + 63) / 64), dim3(64), 0, s, L, out, B, T0, T2, T3, Trec);
    return launch_rc();
}
