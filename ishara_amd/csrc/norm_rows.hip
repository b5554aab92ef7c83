// Row-wise passes over [M, C] activations: LayerNorm forward / backward, the operand maps (Swish, drop-path row scale, dropout mask) and the
// row log-softmax.  Rows are read and written as 16-byte (8 x bf16) or 2 x 16-byte (8 x f32) chunks per lane; all arithmetic is fp32.
#include "kernels.h"


static inline int next_pow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// =====================================================================================
// LayerNorm.  A row is owned by a group of G lanes (G = pow2 >= C/8, <= 64), each lane
// holding one 8-channel chunk in registers (C <= 512) -> exact two-pass statistics.
// =====================================================================================
// sum over aligned groups of G lanes.  Within a 16-lane DPP row the butterfly runs on the VALU (quad_perm / row_half_mirror /
// row_mirror: no LDS round trip); only the steps across rows (G = 32, 64) use ds_bpermute.
template <int CTRL> DEVI float dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int G> DEVI float group_sum(float v) {
    if constexpr (G >= 2) v = dpp_add<0xB1>(v);          // quad_perm [1,0,3,2]: lane ^ 1
    if constexpr (G >= 4) v = dpp_add<0x4E>(v);          // quad_perm [2,3,0,1]: lane ^ 2
    if constexpr (G >= 8) v = dpp_add<0x141>(v);         // row_half_mirror: lane -> 7 - lane within 8 (sums the two quads)
    if constexpr (G >= 16) v = dpp_add<0x140>(v);        // row_mirror: lane -> 15 - lane within 16
#pragma unroll
    for (int o = 16; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <typename T, int G>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, T* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd, int M, int C) {
    constexpr int RPB = 256 / G;
    const int tid = threadIdx.x, gl = tid % G, gr = tid / G;
    const int nch = C >> 3;
    const bool act = gl < nch;
    float ga[8], be[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ga[e] = act ? gamma[gl * 8 + e] : 0.f; be[e] = act ? beta[gl * 8 + e] : 0.f; }
    // four rows in flight per lane group
    const int stride = gridDim.x * RPB;
    for (int row0 = blockIdx.x * RPB + gr; row0 < M; row0 += 4 * stride) {
        float v[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = row0 + u * stride;
            if (act && row < M) load8(x + (size_t)row * C + gl * 8, v[u]);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int row = row0 + u * stride;
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s += v[u][e];
            const float mu = group_sum<G>(s) / (float)C;
            float q = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = act ? v[u][e] - mu : 0.f; q += d * d; }
            const float rs = rsqrtf(group_sum<G>(q) / (float)C + eps);
            if (row < M) {
                if (act) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[u][e] = (v[u][e] - mu) * rs * ga[e] + be[e];
                    store8(y + (size_t)row * C + gl * 8, v[u]);
                }
                if (gl == 0 && mean) { mean[row] = mu; rstd[row] = rs; }
            }
        }
    }
}

int launch_layernorm_fwd(int dt, const void* x, const float* gamma, const float* beta, float eps,
                         void* y, float* mean, float* rstd, int M, int C, hipStream_t s) {
    if (C % 8 != 0 || C > 512) { ishara_set_error("layernorm: C=%d unsupported (need C%%8==0, C<=512)", C); return -1; }
    const int G = next_pow2(C / 8);
    const int rpb = 256 / G;
    // persistent-style grid (2-4 workgroups per CU looping over row batches): at M = 98304 one batch per workgroup (3072
    // workgroups) measured 33.9 us, 512-1536 workgroups 25.7-26.7 us
    const int grid = max(1, min((M + 4 * rpb - 1) / (4 * rpb), 768));
#define LN_F(TT, GG) hipLaunchKernelGGL((layernorm_fwd_kernel<TT, GG>), dim3(grid), dim3(256), 0, s, (const TT*)x, gamma, beta, eps, (TT*)y, mean, rstd, M, C)
#define LN_FG(TT) switch (G) { case 1: LN_F(TT, 1); break; case 2: LN_F(TT, 2); break; case 4: LN_F(TT, 4); break; case 8: LN_F(TT, 8); break; \
                               case 16: LN_F(TT, 16); break; case 32: LN_F(TT, 32); break; default: LN_F(TT, 64); break; }
    if (dt == DT_BF16) { LN_FG(bf16) } else if (dt == DT_F16) { LN_FG(f16) } else { LN_FG(float) }
    return launch_rc();
}

// dx = rstd * (g*dy - mean_c(g*dy) - xhat * mean_c(g*dy*xhat)) (+ resid); dgamma += sum_rows dy*xhat; dbeta += sum_rows dy
template <typename T, int G>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const T* __restrict__ resid,
                                                            T* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            float* __restrict__ partial, int M, int C) {
    constexpr int RPB = 256 / G;
    __shared__ float red[2][256][8];
    const int tid = threadIdx.x, gl = tid % G, gr = tid / G;
    const int nch = C >> 3;
    const bool act = gl < nch;
    float ga[8], dg[8], db[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { ga[e] = act ? gamma[gl * 8 + e] : 0.f; dg[e] = 0.f; db[e] = 0.f; }
    // two rows in flight per group: 4 x 16-byte loads outstanding per lane
    const int stride = gridDim.x * RPB;
    for (int row0 = blockIdx.x * RPB + gr; row0 < M; row0 += 2 * stride) {
        float d[2][8], xv[2][8], o[2][8];
        float mu[2], rs[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = row0 + u * stride;
            const bool ok = act && row < M;
            if (ok) { load8(dy + (size_t)row * C + gl * 8, d[u]); load8(x + (size_t)row * C + gl * 8, xv[u]); }
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) { d[u][e] = 0.f; xv[u][e] = 0.f; }
            }
            if (resid && ok) load8(resid + (size_t)row * C + gl * 8, o[u]);
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[u][e] = 0.f;
            }
            mu[u] = row < M ? mean[row] : 0.f;
            rs[u] = row < M ? rstd[row] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int row = row0 + u * stride;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                xv[u][e] = (act && row < M) ? (xv[u][e] - mu[u]) * rs[u] : 0.f;     // xhat
                dg[e] += d[u][e] * xv[u][e];
                db[e] += d[u][e];
                d[u][e] *= ga[e];
                s1 += d[u][e];
                s2 += d[u][e] * xv[u][e];
            }
            s1 = group_sum<G>(s1) / (float)C;
            s2 = group_sum<G>(s2) / (float)C;
            if (act && row < M) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[u][e] += rs[u] * (d[u][e] - s1 - xv[u][e] * s2);
                store8(dx + (size_t)row * C + gl * 8, o[u]);
            }
        }
    }
    // reduce dgamma/dbeta over the RPB row groups of the block, then one atomic per channel
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[0][tid][e] = dg[e]; red[1][tid][e] = db[e]; }
    __syncthreads();
    if (gr == 0 && act) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = 0.f, b = 0.f;
            for (int r = 0; r < RPB; ++r) { a += red[0][r * G + gl][e]; b += red[1][r * G + gl][e]; }
            if (partial) {      // per-block partial rows [grid][2][C], summed by reduce_slabs (no same-address atomics)
                partial[((size_t)blockIdx.x * 2) * C + gl * 8 + e] = a;
                partial[((size_t)blockIdx.x * 2 + 1) * C + gl * 8 + e] = b;
            } else {
                atomicAdd(dgamma + gl * 8 + e, a);
                atomicAdd(dbeta + gl * 8 + e, b);
            }
        }
    }
}

int launch_layernorm_bwd(int dt, const void* dy, const void* x, const float* mean, const float* rstd,
                         const float* gamma, const void* resid, void* dx, float* dgamma, float* dbeta,
                         float* scratch, int M, int C, hipStream_t s) {
    if (C % 8 != 0 || C > 512) { ishara_set_error("layernorm_bwd: C=%d unsupported", C); return -1; }
    const int G = next_pow2(C / 8);
    const int rpb = 256 / G;
    const int grid = max(1, min((M + 2 * rpb - 1) / (2 * rpb), 1024));     // measured in-model: 512 -> 55 us, 1024 -> 45 us, 2048 -> 49 us
#define LN_B(TT, GG) hipLaunchKernelGGL((layernorm_bwd_kernel<TT, GG>), dim3(grid), dim3(256), 0, s, (const TT*)dy, (const TT*)x, mean, rstd, gamma, (const TT*)resid, (TT*)dx, dgamma, dbeta, scratch, M, C)
#define LN_BG(TT) switch (G) { case 1: LN_B(TT, 1); break; case 2: LN_B(TT, 2); break; case 4: LN_B(TT, 4); break; case 8: LN_B(TT, 8); break; \
                               case 16: LN_B(TT, 16); break; case 32: LN_B(TT, 32); break; default: LN_B(TT, 64); break; }
    if (dt == DT_BF16) { LN_BG(bf16) } else { LN_BG(float) }
    if (scratch) launch_reduce_slabs2(scratch, dgamma, C, dbeta, C, grid, (size_t)2 * C, s);
    return launch_rc();
}
size_t layernorm_bwd_scratch_floats(int C) { return (size_t)2048 * 2 * C; }

// =====================================================================================
// Small streaming passes that materialise an operand transform once so that every GEMM
// (forward, dgrad and wgrad) runs its fast untransformed path:
//   MAP_SWISH    y = swish(x)                  (Squeezeformer conv3 input)
//   MAP_ROWSCALE y = x * rs[row / T]           (drop-path applied to the incoming gradient)
//   MAP_DROPMASK y = x * mask(row, col)        (inverted dropout applied to the incoming gradient)
// =====================================================================================
template <typename T>
__global__ __launch_bounds__(256) void map_rows_kernel(const T* __restrict__ x, T* __restrict__ y, int op, const float* __restrict__ rs,
                                                       DropSpec drop, int M, int Tn, int C) {
    const int nch = C >> 3;
    const int cpr = min(nch, 256), rpb = 256 / cpr;
    const int cl = threadIdx.x % cpr, rl = threadIdx.x / cpr;
    if (rl >= rpb) return;
    for (int row = blockIdx.x * rpb + rl; row < M; row += gridDim.x * rpb) {
        float sc = 1.f;
        uint32_t rk = 0;
        if (op == MAP_ROWSCALE) sc = rs[row / Tn];
        else if (op == MAP_DROPMASK) rk = rng_row_key(drop.key, (uint32_t)row);
        for (int chunk = cl; chunk < nch; chunk += cpr) {
            const size_t off = (size_t)row * C + chunk * 8;
            float v[8];
            load8(x + off, v);
            if (op == MAP_SWISH) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = swishf_(v[e]);
            } else if (op == MAP_ROWSCALE) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= sc;
            } else {
#pragma unroll
                for (int e = 0; e < 8; e += 2) {
                    const uint32_t h = rng_pair(rk, (uint32_t)(chunk * 8 + e));
                    v[e] = (h & 0xffffu) >= drop.thr ? v[e] * drop.scale : 0.f;
                    v[e + 1] = (h >> 16) >= drop.thr ? v[e + 1] * drop.scale : 0.f;
                }
            }
            store8(y + off, v);
        }
    }
}

int launch_map_rows(int dt, int op, const void* x, void* y, const float* rs, DropSpec drop, int M, int T, int C, hipStream_t s) {
    if (C % 8 != 0) { ishara_set_error("map_rows: C%%8 != 0"); return -1; }
    const int cpr = min(C / 8, 256), rpb = 256 / cpr;
    const int grid = max(1, min((M + rpb - 1) / rpb, 4096));
    if (dt == DT_BF16) hipLaunchKernelGGL(map_rows_kernel<bf16>, dim3(grid), dim3(256), 0, s, (const bf16*)x, (bf16*)y, op, rs, drop, M, T, C);
    else if (dt == DT_F16) hipLaunchKernelGGL(map_rows_kernel<f16>, dim3(grid), dim3(256), 0, s, (const f16*)x, (f16*)y, op, rs, drop, M, T, C);
    else hipLaunchKernelGGL(map_rows_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)x, (float*)y, op, rs, drop, M, T, C);
    return launch_rc();
}

// ------------------------------------------------------------------ row log-softmax (the torch Squeezeformer's output layer)
// `F.log_softmax(self.fc(encoder_outputs), dim=-1)` — squeezeformer/model.py:448-449.  One wavefront per row of C fp32 logits
// (C is a class count: tens to a few thousand), exact two-pass form in registers/loop: max, then sum of exp, cross-lane by DPP
// butterflies; a workgroup of 4 waves takes 4 rows per iteration of a grid-stride loop.
__global__ __launch_bounds__(256) void log_softmax_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int M, int C, int ld) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int m = blockIdx.x * 4 + w; m < M; m += gridDim.x * 4) {
        const float* xr = x + (size_t)m * ld;
        float mx = -INFINITY;
        for (int c = lane; c < C; c += 64) mx = fmaxf(mx, xr[c]);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float se = 0.f;
        for (int c = lane; c < C; c += 64) se += __expf(xr[c] - mx);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) se += __shfl_xor(se, o, 64);
        const float lse = mx + __logf(se);
        float* yr = y + (size_t)m * ld;
        for (int c = lane; c < C; c += 64) yr[c] = xr[c] - lse;
        for (int c = C + lane; c < ld; c += 64) yr[c] = 0.f;          // padding columns of the row stride
    }
}
// dx = dy - exp(y) * sum_c dy      (y = the forward's output)
__global__ __launch_bounds__(256) void log_softmax_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx, int M, int C, int ld) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int m = blockIdx.x * 4 + w; m < M; m += gridDim.x * 4) {
        const float* gr = dy + (size_t)m * ld;
        const float* yr = y + (size_t)m * ld;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += gr[c];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        float* dr = dx + (size_t)m * ld;
        for (int c = lane; c < C; c += 64) dr[c] = gr[c] - __expf(yr[c]) * s;
        for (int c = C + lane; c < ld; c += 64) dr[c] = 0.f;
    }
}
int launch_log_softmax_fwd(const float* x, float* y, int M, int C, int ld, hipStream_t s) {
    if (M < 1 || C < 1 || ld < C) { ishara_set_error("log_softmax: M=%d C=%d ld=%d", M, C, ld); return -1; }
    hipLaunchKernelGGL(log_softmax_fwd_kernel, dim3(max(1, min((M + 3) / 4, 2048))), dim3(256), 0, s, x, y, M, C, ld);
    return launch_rc();
}
int launch_log_softmax_bwd(const float* dy, const float* y, float* dx, int M, int C, int ld, hipStream_t s) {
    if (M < 1 || C < 1 || ld < C) { ishara_set_error("log_softmax: M=%d C=%d ld=%d", M, C, ld); return -1; }
    hipLaunchKernelGGL(log_softmax_bwd_kernel, dim3(max(1, min((M + 3) / 4, 2048))), dim3(256), 0, s, dy, y, dx, M, C, ld);
    return launch_rc();
}