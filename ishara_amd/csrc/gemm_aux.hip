// Small kernels around the GEMMs: weight shadows, the bf16 / fp16 row packer of the stem input and the narrow classifier.
#include "gemm_tile.h"

// ---------------------------------------------------------------------------------
// weight shadows: Wt[n][k] = W[k][n] (ld ldt) and Wn[k][n] = W[k][n] (ld ldn), zero padded
// by a preceding memset of the whole shadow arena.
// ---------------------------------------------------------------------------------
template <typename TM>
__global__ void make_shadow_kernel(const float* __restrict__ W, int K, int N, TM* __restrict__ Wt, int ldt, TM* __restrict__ Wn, int ldn) {
    __shared__ float tile[32][33];
    const int k0 = blockIdx.y * 32, n0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, n = n0 + tx;
        float v = 0.f;
        if (k < K && n < N) { v = W[(size_t)k * N + n]; if (Wn) Wn[(size_t)k * ldn + n] = from_f<TM>(v); }
        tile[r][tx] = v;
    }
    __syncthreads();
    if (Wt) {
        for (int r = ty; r < 32; r += 8) {
            const int n = n0 + r, k = k0 + tx;
            if (k < K && n < N) Wt[(size_t)n * ldt + k] = from_f<TM>(tile[tx][r]);
        }
    }
}

// all weight shadows of the model in ONE launch: block -> (weight, 32x32 tile) through a descriptor table in device memory
template <typename TM>
__global__ void make_shadow_batched_kernel(const ShadowDesc* __restrict__ tab, int ntab) {
    __shared__ float tile[32][33];
    int wi = 0;
    for (int hi = ntab; hi - wi > 1;) {       // the weight this tile belongs to: binary search over the descriptors' first tiles (a linear walk
        const int mid = (wi + hi) >> 1;       // was up to ntab dependent loads per block: 0.7 ms per step for configs[3]'s 88 M parameters)
        if ((int)blockIdx.x >= tab[mid].tile0) wi = mid; else hi = mid;
    }
    const ShadowDesc d = tab[wi];
    const int lt = blockIdx.x - d.tile0;
    const int k0 = (lt / d.tiles_n) * 32, n0 = (lt % d.tiles_n) * 32;
    TM* Wt = reinterpret_cast<TM*>(d.Wt);
    TM* Wn = reinterpret_cast<TM*>(d.Wn);
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        const int k = k0 + r, n = n0 + tx;
        float v = 0.f;
        if (k < d.K && n < d.N) { v = d.W[(size_t)k * d.N + n]; if (Wn) Wn[(size_t)k * d.ldn + n] = from_f<TM>(v); }
        tile[r][tx] = v;
    }
    __syncthreads();
    if (Wt) {
        for (int r = ty; r < 32; r += 8) {
            const int n = n0 + r, k = k0 + tx;
            if (k < d.K && n < d.N) Wt[(size_t)n * d.ldt + k] = from_f<TM>(tile[tx][r]);
        }
    }
}
int launch_make_shadow_batched(int dtM, const ShadowDesc* tab, int ntab, int total_tiles, hipStream_t s) {
    if (ntab <= 0 || total_tiles <= 0) return 0;
    if (dtM == DT_BF16) hipLaunchKernelGGL(make_shadow_batched_kernel<bf16>, dim3(total_tiles), dim3(256), 0, s, tab, ntab);
    else if (dtM == DT_F16) hipLaunchKernelGGL(make_shadow_batched_kernel<f16>, dim3(total_tiles), dim3(256), 0, s, tab, ntab);
    else hipLaunchKernelGGL(make_shadow_batched_kernel<float>, dim3(total_tiles), dim3(256), 0, s, tab, ntab);
    return launch_rc();
}

int launch_make_shadow(int dtM, const float* W, int K, int N, void* Wt, int ldt, void* Wn, int ldn, hipStream_t s) {
    dim3 grid((N + 31) / 32, (K + 31) / 32);
    if (dtM == DT_BF16) hipLaunchKernelGGL(make_shadow_kernel<bf16>, grid, dim3(256), 0, s, W, K, N, (bf16*)Wt, ldt, (bf16*)Wn, ldn);
    else if (dtM == DT_F16) hipLaunchKernelGGL(make_shadow_kernel<f16>, grid, dim3(256), 0, s, W, K, N, (f16*)Wt, ldt, (f16*)Wn, ldn);
    else hipLaunchKernelGGL(make_shadow_kernel<float>, grid, dim3(256), 0, s, W, K, N, (float*)Wt, ldt, (float*)Wn, ldn);
    return launch_rc();
}

// xb[M, Kp] (bf16) = x[M, F] (f32) zero padded: the stem's input rows as an MFMA operand (the f32-A GEMM kernels round the
// same way while staging; done once here, the stem Dense and its wgrad run on the bf16 fast paths with K = Kp)
template <typename TM>
__global__ __launch_bounds__(256) void pack_rows_bf16_kernel(const float* __restrict__ x, TM* __restrict__ xb, int M, int F, int Kp) {
    const int cpr = Kp >> 3;                                   // 16-byte output chunks per row
    const size_t total = (size_t)M * cpr;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / cpr;
        const int c0 = (int)(i - row * cpr) * 8;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const float* src = x + row * F + c0;
        if (c0 + 4 <= F) { const float4 a = *reinterpret_cast<const float4*>(src); v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; }
        if (c0 + 8 <= F) { const float4 a = *reinterpret_cast<const float4*>(src + 4); v[4] = a.x; v[5] = a.y; v[6] = a.z; v[7] = a.w; }
        *reinterpret_cast<u32x4*>(xb + row * Kp + c0) = pack_chunk<TM, 8>(v);
    }
}
template <typename TM>
__global__ __launch_bounds__(256) void dense_narrow_kernel(const TM* __restrict__ A, const TM* __restrict__ Wt, int ldt, const float* __restrict__ bias,
                                                           float* __restrict__ C, int M, int N, int K) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int m0 = (blockIdx.x * 4 + wid) * 4;                  // this wave's 4 rows
    const int n = min(lane, N - 1);
    const TM* wrow = Wt + (size_t)n * ldt;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int mr[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mr[r] = min(m0 + r, M - 1);
    for (int k = 0; k < K; k += 32) {                            // 4 weight chunks and 16 operand chunks (wave-uniform addresses) in flight
        u32x4 w[4], a[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            w[u] = *reinterpret_cast<const u32x4*>(wrow + k + 8 * u);
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r][u] = *reinterpret_cast<const u32x4*>(A + (size_t)mr[r] * K + k + 8 * u);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            typedef __attribute__((ext_vector_type(8))) TM v8;
            const v8 wv = __builtin_bit_cast(v8, w[u]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const v8 av = __builtin_bit_cast(v8, a[r][u]);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[r] += (float)av[e] * (float)wv[e];
            }
        }
    }
    if (lane < N) {
        const float b = bias ? bias[lane] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) if (m0 + r < M) C[(size_t)(m0 + r) * N + lane] = acc[r] + b;
    }
}
int launch_dense_narrow(int dt, const void* A, const void* Wt, int ldt, const float* bias, float* C, int M, int N, int K, hipStream_t s) {
    if (!dt_is16(dt) || N < 1 || N > 64 || K % 32 != 0 || ldt % 8 != 0 || ((uintptr_t)A) % 16 != 0 || ((uintptr_t)Wt) % 16 != 0) { ishara_set_error("dense_narrow: N=%d K=%d unsupported", N, K); return -1; }
    const dim3 grid((M + 15) / 16);
    if (dt == DT_F16) hipLaunchKernelGGL(dense_narrow_kernel<f16>, grid, dim3(256), 0, s, (const f16*)A, (const f16*)Wt, ldt, bias, C, M, N, K);
    else hipLaunchKernelGGL(dense_narrow_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)A, (const bf16*)Wt, ldt, bias, C, M, N, K);
    return launch_rc();
}

int launch_pack_rows_bf16(const float* x, void* xb, int M, int F, int Kp, hipStream_t s, int dt) {
    if (F % 4 != 0 || Kp % 8 != 0 || Kp < F || ((uintptr_t)x) % 16 != 0) { ishara_set_error("pack_rows_bf16: F=%d Kp=%d unsupported", F, Kp); return -1; }
    const int grid = (int)std::min<size_t>(2048, ((size_t)M * (Kp >> 3) + 255) / 256);
    if (dt == DT_F16) hipLaunchKernelGGL(pack_rows_bf16_kernel<f16>, dim3(grid), dim3(256), 0, s, x, (f16*)xb, M, F, Kp);
    else hipLaunchKernelGGL(pack_rows_bf16_kernel<bf16>, dim3(grid), dim3(256), 0, s, x, (bf16*)xb, M, F, Kp);
    return launch_rc();
}
