// BatchNorm, ECA and Squeeze-Excite around the depthwise conv: per-sample reductions over time, BatchNorm finalize / backward, the ECA and SE
// gates ([B, C]-sized, one workgroup per sample) and the affine passes that apply them.  Activations are [B*T, C] row-major (channel fastest),
// read and written as 16-byte chunks per lane; all arithmetic is fp32, sums across samples fp64.
#include "kernels.h"

// =====================================================================================
// per-sample reductions over time:  S1[b,c] += sum_t dy ; S2[b,c] += sum_t dy * o,
// o = other (optionally normalised (other-mean)*rstd).  grid = (B, time splits).
// =====================================================================================
// grid = (B, ceil(C / 128)): a workgroup owns 128 channels of one sample — 16 chunk lanes (8 channels, 16 bytes) x 16 row
// lanes, four rows in flight per lane — and WRITES its sums (no atomics, no zero-fill launches).
template <typename T>
__global__ __launch_bounds__(256) void sample_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ other,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            float* __restrict__ S1, float* __restrict__ S2, int B, int Tn, int C) {
    __shared__ float red[2][16][16][8];
    const int tid = threadIdx.x, cl = tid & 15, rl = tid >> 4;
    const int b = blockIdx.x;
    const int chunk = blockIdx.y * 16 + cl;
    const bool act = chunk * 8 < C;
    float a[8], q[8], mu[8], rs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { a[e] = 0.f; q[e] = 0.f; mu[e] = (act && mean) ? mean[chunk * 8 + e] : 0.f; rs[e] = (act && mean) ? rstd[chunk * 8 + e] : 1.f; }
    if (act) {
        for (int t0 = rl; t0 < Tn; t0 += 64) {
            float d[4][8], o[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int t = min(t0 + 16 * u, Tn - 1);
                const size_t off = ((size_t)b * Tn + t) * C + chunk * 8;
                load8(dy + off, d[u]);
                if (other) load8(other + off, o[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (t0 + 16 * u < Tn) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { a[e] += d[u][e]; if (other) q[e] += d[u][e] * ((o[u][e] - mu[e]) * rs[e]); }
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[0][rl][cl][e] = a[e]; red[1][rl][cl][e] = q[e]; }
    __syncthreads();
    if (tid < 128) {            // thread -> channel tid of the 128
        const int c = blockIdx.y * 128 + tid;
        if (c < C) {
            float sa = 0.f, sq = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { sa += red[0][r][tid >> 3][tid & 7]; sq += red[1][r][tid >> 3][tid & 7]; }
            S1[(size_t)b * C + c] = sa;
            if (S2) S2[(size_t)b * C + c] = sq;
        }
    }
}

int launch_sample_reduce(int dt, const void* dy, const void* other, const float* mean, const float* rstd,
                         float* S1, float* S2, int B, int T, int C, hipStream_t s) {
    if (C % 8 != 0) { ishara_set_error("sample_reduce: C%%8 != 0"); return -1; }
    dim3 grid(B, (C + 127) / 128);
    if (dt == DT_BF16) hipLaunchKernelGGL(sample_reduce_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)dy, (const bf16*)other, mean, rstd, S1, S2, B, T, C);
    else if (dt == DT_F16) hipLaunchKernelGGL(sample_reduce_kernel<f16>, grid, dim3(256), 0, s, (const f16*)dy, (const f16*)other, mean, rstd, S1, S2, B, T, C);
    else hipLaunchKernelGGL(sample_reduce_kernel<float>, grid, dim3(256), 0, s, (const float*)dy, (const float*)other, mean, rstd, S1, S2, B, T, C);
    return launch_rc();
}

// =====================================================================================
// BatchNorm finalize from per-sample sums [nb, C] (fp64 accumulation across samples)
// =====================================================================================
// block = FIN_CL channels x FIN_BL sample lanes (1024 threads); fp64 accumulation across samples.  16 x 64 instead of
// 64 x 16: C = 512 gives 32 workgroups with 4 samples per thread instead of 8 with 16 (these [B, C] passes are latency
// bound).  A wave holds 4 sample lanes x 16 channels: two shuffles fold the
// lanes, then the 16 waves are summed through LDS in a fixed order.
#define FIN_CL 16
#define FIN_BL 64
#define FIN_NW (FIN_CL * FIN_BL / 64)
DEVI double fin_fold(double v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__global__ __launch_bounds__(1024) void bn_finalize_kernel(const float* __restrict__ ssum, const float* __restrict__ ssq, int nb, float count,
                                   const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float momentum,
                                   float* __restrict__ mmean, float* __restrict__ mvar, int training,
                                   float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ a, float* __restrict__ bsh, int C, float var_corr, int stride) {
    // stride: floats between consecutive rows of ssum / ssq (C: [nb, C] arrays; 2C: the depthwise conv's partial statistic rows [nb][2][C] read in place)
    __shared__ double rs_[FIN_NW][FIN_CL], rq_[FIN_NW][FIN_CL];
    const int cl = threadIdx.x & (FIN_CL - 1), bl = threadIdx.x / FIN_CL, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * FIN_CL + cl;
    double s = 0.0, q = 0.0;
    if (training && c < C)
        for (int b = bl; b < nb; b += FIN_BL) { s += (double)ssum[(size_t)b * stride + c]; q += (double)ssq[(size_t)b * stride + c]; }
    s = fin_fold(s); q = fin_fold(q);
    if ((threadIdx.x & 63) < FIN_CL) { rs_[wv][cl] = s; rq_[wv][cl] = q; }
    __syncthreads();
    if (bl != 0 || c >= C) return;
    float mu, var;
    if (training) {
        for (int i = 1; i < FIN_NW; ++i) { s += rs_[i][cl]; q += rq_[i][cl]; }
        const double m = s / (double)count;
        double v = q / (double)count - m * m;
        if (v < 0.0) v = 0.0;
        mu = (float)m; var = (float)v;
        mmean[c] = mmean[c] * momentum + mu * (1.f - momentum);
        mvar[c] = mvar[c] * momentum + var * var_corr * (1.f - momentum);
    } else { mu = mmean[c]; var = mvar[c]; }
    const float rs = rsqrtf(var + eps);
    mean[c] = mu; rstd[c] = rs;
    const float aa = gamma[c] * rs;
    a[c] = aa; bsh[c] = beta[c] - mu * aa;
}

int launch_bn_finalize(const float* ssum, const float* ssq, int nb, float count, const float* gamma, const float* beta,
                          float eps, float momentum, float* moving_mean, float* moving_var, int training,
                          float* mean, float* rstd, float* a, float* b, int C, hipStream_t s, float var_corr, int stride) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + FIN_CL - 1) / FIN_CL), dim3(FIN_CL * FIN_BL), 0, s, ssum, ssq, nb, count, gamma, beta, eps, momentum,
                       moving_mean, moving_var, training, mean, rstd, a, b, C, var_corr, stride ? stride : C);
    return launch_rc();
}

// =====================================================================================
// ECA gate on [B,C] (one workgroup per sample)
// =====================================================================================
// inf.part != nullptr (inference): the kernel also does what two launches did before it — the sum of the depthwise conv's partial statistic
// rows (the sample's channel sums over time) and the BatchNorm constants from the moving statistics (a = gamma * rsqrt(mv + eps),
// b = beta - mm * a) — so a Conv1DBlock's forward is 4 launches instead of 6 (configs[4]: B = 1, every launch is ~9 us of latency)
// inf.part != nullptr with inf.mm == nullptr (training, round 3): the partial rows are summed here too (the per-sample sums go to inf.gap_out
// for the backward pass — the stats_reduce launch is gone), the BatchNorm constants come from bn_finalize (batch statistics) as before
struct EcaInfer { const float* part = nullptr; int prows = 0; const float* mm = nullptr; const float* mv = nullptr; const float* gamma = nullptr; const float* beta = nullptr; float eps = 0.f;
                  float* gap_out = nullptr; };
__global__ __launch_bounds__(1024) void eca_fwd_kernel(const float* __restrict__ gap, const float* __restrict__ a, const float* __restrict__ bsh,
                                                      const float* __restrict__ w5, float invT, float* __restrict__ gn,
                                                      float* __restrict__ sg, float* __restrict__ P, float* __restrict__ Q, int C, float* __restrict__ rs, DropSpec dp, int dp_fold, EcaInfer inf) {
    extern __shared__ float sh[];   // [C + 4] (+ [C] a, [C] b for the inference form)
    float* al = sh + C + 4;
    float* bl = al + C;
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C + 4; c += blockDim.x) {
        const int cc = c - 2;
        float g = 0.f;
        if (cc >= 0 && cc < C) {
            if (inf.part) {
                const float* p = inf.part + ((size_t)b * inf.prows * 2) * C + cc;
                float s0 = 0.f;
                for (int r = 0; r < inf.prows; ++r) s0 += p[(size_t)(2 * r) * C];
                if (inf.mm) {
                    const float aa = inf.gamma[cc] * rsqrtf(inf.mv[cc] + inf.eps), bb = inf.beta[cc] - inf.mm[cc] * aa;
                    al[cc] = aa; bl[cc] = bb;
                    g = aa * s0 * invT + bb;
                } else {
                    inf.gap_out[(size_t)b * C + cc] = s0;
                    g = a[cc] * s0 * invT + bsh[cc];
                }
            } else g = a[cc] * gap[(size_t)b * C + cc] * invT + bsh[cc];
            gn[(size_t)b * C + cc] = g;
        }
        sh[c] = g;
    }
    __syncthreads();
    if (inf.part && inf.mm) { a = al; bsh = bl; }
    const float w0 = w5[0], w1 = w5[1], w2 = w5[2], w3 = w5[3], w4 = w5[4];
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const float z = w0 * sh[c] + w1 * sh[c + 1] + w2 * sh[c + 2] + w3 * sh[c + 3] + w4 * sh[c + 4];
        const float sv = sigmoidf_(z);
        sg[(size_t)b * C + c] = sv;
        // drop-path scale of this sample (c5:82-83, noise_shape (None,1,1)): drawn here (dp.thr != 0), published in rs[b] for the GEMM
        // epilogues and the backward pass, and folded into P, Q when `rs` is given
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

int launch_eca_fwd(const float* gap, const float* a, const float* b, const float* w5, float invT,
                   float* gn, float* sgate, float* P, float* Q, int B, int C, hipStream_t s, float* rs, DropSpec dp, int dp_fold) {
    hipLaunchKernelGGL(eca_fwd_kernel, dim3(B), dim3(256), (C + 4) * sizeof(float), s, gap, a, b, w5, invT, gn, sgate, P, Q, C, rs, dp, dp_fold, EcaInfer{});
    return launch_rc();
}
// training form over the depthwise conv's partial statistic rows: sums them per sample (-> gap_out [B, C]) and gates with bn_finalize's constants
int launch_eca_fwd_part(const float* part, int prows, float* gap_out, const float* a, const float* b, const float* w5, float invT,
                        float* gn, float* sgate, float* P, float* Q, int B, int C, hipStream_t s, float* rs, DropSpec dp, int dp_fold) {
    EcaInfer inf; inf.part = part; inf.prows = prows; inf.gap_out = gap_out;
    hipLaunchKernelGGL(eca_fwd_kernel, dim3(B), dim3(256), (3 * C + 4) * sizeof(float), s, (const float*)nullptr, a, b, w5, invT, gn, sgate, P, Q, C, rs, dp, dp_fold, inf);
    return launch_rc();
}
int launch_eca_fwd_infer(const float* part, int prows, const float* mm, const float* mv, const float* gamma, const float* beta, float eps, const float* w5, float invT,
                         float* gn, float* sgate, float* P, float* Q, int B, int C, hipStream_t s) {
    EcaInfer inf; inf.part = part; inf.prows = prows; inf.mm = mm; inf.mv = mv; inf.gamma = gamma; inf.beta = beta; inf.eps = eps;
    const int threads = B <= 8 ? (C + 4 > 512 ? 1024 : 512) : 256;      // a clip or a few: a thread per channel (one workgroup per sample is all the parallelism there is)
    hipLaunchKernelGGL(eca_fwd_kernel, dim3(B), dim3(threads), (3 * C + 4) * sizeof(float), s, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, w5, invT, gn, sgate, P, Q, C,
                       (float*)nullptr, DropSpec{0, 0, 1.f}, 0, inf);
    return launch_rc();
}

// =====================================================================================
// y = x*P[b,c] + Q[b,c] (+resid)  /  y = x*a[c] + b[c]
// =====================================================================================
// grid = (row blocks, samples); a thread keeps one 8-channel chunk, so the per-sample /
// per-channel coefficients are loaded once and the row loop is pure 16-byte streaming.
template <typename T>
__global__ __launch_bounds__(256) void affine_kernel(const T* __restrict__ x, const float* __restrict__ P, const float* __restrict__ Q,
                                                     const T* __restrict__ resid, T* __restrict__ y, int Tn, int C, int per_sample) {
    const int nch = C >> 3;
    const int cpr = min(nch, 256), rpb = 256 / cpr;
    const int cl = threadIdx.x % cpr, rl = threadIdx.x / cpr;
    const int b = blockIdx.y;
    if (rl >= rpb) return;
    for (int chunk = cl; chunk < nch; chunk += cpr) {
        const float* pp = P + (per_sample ? (size_t)b * C : 0) + chunk * 8;
        float p[8], q[8];
        load8(pp, p);
        if (Q) load8(Q + (per_sample ? (size_t)b * C : 0) + chunk * 8, q);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) q[e] = 0.f;
        }
        for (int t = blockIdx.x * rpb + rl; t < Tn; t += gridDim.x * rpb) {
            const size_t off = ((size_t)b * Tn + t) * C + chunk * 8;
            float v[8];
            load8(x + off, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] * p[e] + q[e];
            if (resid) {
                float r[8];
                load8(resid + off, r);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += r[e];
            }
            store8(y + off, v);
        }
    }
}

static int run_affine(int dt, const void* x, const float* P, const float* Q, const void* resid, void* y, int B, int T, int C, int per_sample, hipStream_t s) {
    if (C % 8 != 0) { ishara_set_error("affine: C%%8 != 0"); return -1; }
    const int cpr = min(C / 8, 256), rpb = 256 / cpr;
    int gx = (T + rpb - 1) / rpb;
    const int cap = max(1, 4096 / max(B, 1));
    if (gx > cap) gx = cap;
    dim3 grid(gx, B);
    if (dt == DT_BF16) hipLaunchKernelGGL(affine_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)x, P, Q, (const bf16*)resid, (bf16*)y, T, C, per_sample);
    else if (dt == DT_F16) hipLaunchKernelGGL(affine_kernel<f16>, grid, dim3(256), 0, s, (const f16*)x, P, Q, (const f16*)resid, (f16*)y, T, C, per_sample);
    else hipLaunchKernelGGL(affine_kernel<float>, grid, dim3(256), 0, s, (const float*)x, P, Q, (const float*)resid, (float*)y, T, C, per_sample);
    return launch_rc();
}
int launch_sample_affine(int dt, const void* x, const float* P, const float* Q, const void* resid, void* y, int B, int T, int C, hipStream_t s) {
    return run_affine(dt, x, P, Q, resid, y, B, T, C, 1, s);
}
int launch_col_affine(int dt, const void* x, const float* a, const float* b, void* y, int M, int C, hipStream_t s) {
    // rows are independent: present them as min(M, 256) pseudo-samples for grid parallelism
    int Bp = 1;
    for (int cand = 256; cand >= 1; cand >>= 1) if (M % cand == 0) { Bp = cand; break; }
    return run_affine(dt, x, a, b, nullptr, y, Bp, M / Bp, C, 0, s);
}

// =====================================================================================
// BatchNorm backward pieces
// =====================================================================================
// Conv1DBlock (BN -> ECA): step 1, per sample.  E <- dgn[b,c]; dw5 += sum dz*gn(shifted)
// grid = (B, channel chunks of CC): a workgroup owns CC channels of one sample (the 5-tap channel convolution reaches 2 channels into the
// neighbouring chunks).  ps.G != nullptr (PsaStats, kernels.h): S1, S2 are first computed from what the per-sample-affine weight-gradient
// GEMM emitted — S1[c] = rs * sum_n Wt[n,c] G[n], S2[c] = rstd[c] * (rs * sum_p Rpart[p][c] - mean[c] * S1[c]) — for the chunk and one
// 8-channel group of halo on each side (kept in LDS; only the chunk's own values are written out): thread (cg, w) takes 8 channels (16-byte
// weight loads, channel = fast index) and a quarter of the N weight rows, 32 loads in flight (one thread per channel over all N sat on load
// latency: 37 us as a kernel of its own; one workgroup per sample over all channels: 32 us at C = 1024, B = 64)
__global__ __launch_bounds__(256) void eca_bwd_sample_kernel(float* __restrict__ S1, float* __restrict__ S2,
                                                             const float* __restrict__ gn, const float* __restrict__ sg,
                                                             const float* __restrict__ w5, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ E,
                                                             float* __restrict__ dw5part, int C, int CC, PsaStats ps) {
    extern __shared__ float sh[];
    const int CH = CC + 16;
    float* dz = sh;                 // [CC + 4]: channel c_lo - 2 + i
    float* g = dz + CC + 4;         // [CC + 4]
    float* s1l = g + CC + 4;        // [CH]: channel c_lo - 8 + i
    float* s2l = s1l + CH;
    float* gl = s2l + CH;           // [N]
    __shared__ float wred[5][4];
    const int b = blockIdx.x, c_lo = (int)blockIdx.y * CC, c_hi = min(C, c_lo + CC);
    if (ps.G) {
        const int N = ps.N, cg = threadIdx.x & 63, w = threadIdx.x >> 6;
        float* part = gl + N;       // [4][CH]
        for (int n = threadIdx.x; n < N; n += 256) gl[n] = ps.G[(size_t)b * N + n];
        const bf16* Wt = reinterpret_cast<const bf16*>(ps.Wt);
        const int nq = (N + 3) / 4, nbeg = w * nq, nend = min(N, nbeg + nq);
        __syncthreads();
        for (int i0 = cg * 8; i0 < CH; i0 += 512) {
            const int c0 = c_lo - 8 + i0;
            float a[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] = 0.f;
            if (c0 >= 0 && c0 < C) {
                for (int n = nbeg; n < nend; n += 32) {
                    bf16x8 wv[32];
#pragma unroll
                    for (int u = 0; u < 32; ++u) wv[u] = *reinterpret_cast<const bf16x8*>(Wt + (size_t)min(n + u, nend - 1) * ps.ldt + c0);
#pragma unroll
                    for (int u = 0; u < 32; ++u) {
                        const float gv = n + u < nend ? gl[n + u] : 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) a[e] += (float)wv[u][e] * gv;
                    }
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) part[w * CH + i0 + e] = a[e];
        }
        __syncthreads();
        const float r = ps.rs ? ps.rs[b] : 1.f;
        for (int i = threadIdx.x; i < CH; i += 256) {
            const int c = c_lo - 8 + i;
            float s1 = 0.f, s2 = 0.f;
            if (c >= 0 && c < C) {
                float R = 0.f;
                for (int p = 0; p < ps.nparts; ++p) R += ps.Rpart[((size_t)b * ps.nparts + p) * C + c];
                s1 = r * (part[i] + part[CH + i] + part[2 * CH + i] + part[3 * CH + i]);
                s2 = ps.rstd[c] * (r * R - ps.mean[c] * s1);
                if (c >= c_lo && c < c_hi) { S1[(size_t)b * C + c] = s1; S2[(size_t)b * C + c] = s2; }
            }
            s1l[i] = s1; s2l[i] = s2;
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < CC + 4; i += blockDim.x) {
        const int cc = c_lo - 2 + i;
        float z = 0.f, gg = 0.f;
        if (cc >= 0 && cc < C) {
            const size_t idx = (size_t)b * C + cc;
            const float s1 = ps.G ? s1l[i + 6] : S1[idx], s2 = ps.G ? s2l[i + 6] : S2[idx];
            const float ds = gamma[cc] * s2 + beta[cc] * s1;
            const float sv = sg[idx];
            z = ds * sv * (1.f - sv);
            gg = gn[idx];
        }
        dz[i] = z; g[i] = gg;
    }
    __syncthreads();
    float wp[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = c_lo + threadIdx.x; c < c_hi; c += blockDim.x) {
        const int li = c - c_lo;
        // dgn[c] = sum_j w5[j] * dz(channel c - j + 2)  -> local index li - j + 4
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 5; ++j) acc += w5[j] * dz[li - j + 4];
        E[(size_t)b * C + c] = acc;
        // dw5[j] += dz(c) * gn(c + j - 2) -> local index li + j
        const float z = dz[li + 2];
#pragma unroll
        for (int j = 0; j < 5; ++j) wp[j] += z * g[li + j];
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 5; ++j) { const float v = wave_sum(wp[j]); if (lane == 0) wred[j][wid] = v; }
    __syncthreads();
    if (threadIdx.x < 5) dw5part[((size_t)b * gridDim.y + blockIdx.y) * 8 + threadIdx.x] = wred[threadIdx.x][0] + wred[threadIdx.x][1] + wred[threadIdx.x][2] + wred[threadIdx.x][3];   // summed in order by the channel kernel
}

// step 2, per channel (FIN_CL channels x FIN_BL sample lanes per block): dgamma, dbeta, Fc; E[b,c] <- dgn/T - dbeta/Mtot
__global__ __launch_bounds__(1024) void eca_bn_bwd_channel_kernel(const float* __restrict__ S1, const float* __restrict__ S2, const float* __restrict__ gap,
                                          const float* __restrict__ sg, const float* __restrict__ mean, const float* __restrict__ rstd,
                                          float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ E, float* __restrict__ Fc,
                                          const float* __restrict__ dw5part, int nparts5, float* __restrict__ dw5, int B, int Tn, int C) {
    __shared__ double rg_[FIN_NW][FIN_CL], rb_[FIN_NW][FIN_CL];
    __shared__ float eb_[FIN_CL];
    if (blockIdx.x == 0 && threadIdx.x < 5 * 64) {      // ECA tap gradient: per-(sample, chunk) partials of step 1, summed in a fixed order (wave j = tap j)
        const int j = threadIdx.x >> 6, l = threadIdx.x & 63;
        float a = 0.f;
        for (int b = l; b < nparts5; b += 64) a += dw5part[(size_t)b * 8 + j];
        a = wave_sum(a);
        if (l == 0) dw5[j] += a;
    }
    const int cl = threadIdx.x & (FIN_CL - 1), bl = threadIdx.x / FIN_CL, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * FIN_CL + cl;
    const bool act = c < C;
    const float invT = 1.f / (float)Tn, mu = act ? mean[c] : 0.f, rs = act ? rstd[c] : 0.f;
    double dg = 0.0, db = 0.0;
    if (act)
        for (int b = bl; b < B; b += FIN_BL) {
            const size_t i = (size_t)b * C + c;
            const float ghat = (gap[i] * invT - mu) * rs;
            dg += (double)(sg[i] * S2[i] + E[i] * ghat);
            db += (double)(sg[i] * S1[i] + E[i]);
        }
    dg = fin_fold(dg); db = fin_fold(db);
    if ((threadIdx.x & 63) < FIN_CL) { rg_[wv][cl] = dg; rb_[wv][cl] = db; }
    __syncthreads();
    const float mtot = (float)B * (float)Tn;
    if (bl == 0 && act) {
        for (int i = 1; i < FIN_NW; ++i) { dg += rg_[i][cl]; db += rb_[i][cl]; }
        dgamma[c] += (float)dg;
        dbeta[c] += (float)db;
        Fc[c] = (float)dg / mtot;
        eb_[cl] = (float)db / mtot;
    }
    __syncthreads();
    if (act) {
        const float eb = eb_[cl];
        for (int b = bl; b < B; b += FIN_BL) { const size_t i = (size_t)b * C + c; E[i] = E[i] * invT - eb; }
    }
}

// step 2 with per-clip frame lengths (frame_mask.hip): the gate pooled BN(h2) over the n_b valid frames, so `gap` holds that masked MEAN
// (at n_b = 0 the pooled value is the constant 0) and the gate's gradient reaches the valid frames only.  The constant of the unmasked kernel splits in two:
// E[b,c] <- dgn / n_b (frames t < n_b) and Ecol[c] = -dbeta / Mtot (every frame); dgamma, dbeta, Fc as above
__global__ __launch_bounds__(1024) void eca_bn_bwd_channel_len_kernel(const float* __restrict__ S1, const float* __restrict__ S2, const float* __restrict__ gap,
                                          const float* __restrict__ sg, const float* __restrict__ mean, const float* __restrict__ rstd,
                                          float* __restrict__ dgamma, float* __restrict__ dbeta, float* __restrict__ E, float* __restrict__ Ecol, float* __restrict__ Fc,
                                          const float* __restrict__ dw5part, int nparts5, float* __restrict__ dw5, const int* __restrict__ frame_len, int B, int Tn, int C) {
    __shared__ double rg_[FIN_NW][FIN_CL], rb_[FIN_NW][FIN_CL];
    if (blockIdx.x == 0 && threadIdx.x < 5 * 64) {      // ECA tap gradient, as in the unmasked kernel
        const int j = threadIdx.x >> 6, l = threadIdx.x & 63;
        float a = 0.f;
        for (int b = l; b < nparts5; b += 64) a += dw5part[(size_t)b * 8 + j];
        a = wave_sum(a);
        if (l == 0) dw5[j] += a;
    }
    const int cl = threadIdx.x & (FIN_CL - 1), bl = threadIdx.x / FIN_CL, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * FIN_CL + cl;
    const bool act = c < C;
    const float mu = act ? mean[c] : 0.f, rs = act ? rstd[c] : 0.f;
    double dg = 0.0, db = 0.0;
    if (act)
        for (int b = bl; b < B; b += FIN_BL) {
            const size_t i = (size_t)b * C + c;
            const float ghat = (gap[i] - mu) * rs;
            const float ev = attn_key_count(frame_len, b, Tn) > 0 ? E[i] : 0.f;      // n_b = 0: the pooled value is the constant 0, its gradient reaches nothing
            dg += (double)(sg[i] * S2[i] + ev * ghat);
            db += (double)(sg[i] * S1[i] + ev);
        }
    dg = fin_fold(dg); db = fin_fold(db);
    if ((threadIdx.x & 63) < FIN_CL) { rg_[wv][cl] = dg; rb_[wv][cl] = db; }
    __syncthreads();
    const float mtot = (float)B * (float)Tn;
    if (bl == 0 && act) {
        for (int i = 1; i < FIN_NW; ++i) { dg += rg_[i][cl]; db += rb_[i][cl]; }
        dgamma[c] += (float)dg;
        dbeta[c] += (float)db;
        Fc[c] = (float)dg / mtot;
        Ecol[c] = -((float)db / mtot);
    }
    if (act)
        for (int b = bl; b < B; b += FIN_BL) {
            const int n = attn_key_count(frame_len, b, Tn);
            const size_t i = (size_t)b * C + c;
            E[i] = n > 0 ? E[i] * (1.f / (float)n) : 0.f;
        }
}

int launch_eca_bn_bwd_finalize(float* S1, float* S2, const float* gap, const float* gn, const float* sgate,
                               const float* w5, const float* gamma, const float* beta, const float* mean, const float* rstd,
                               float* dgamma, float* dbeta, float* dw5, float* E, float* Fc, float* dw5part, int B, int T, int C, hipStream_t s, const PsaStats* ps,
                               const int* frame_len, float* Ecol) {
    if (frame_len) {
        if (ps || !Ecol) { ishara_set_error("eca_bn_bwd_finalize: frame lengths go with S1 / S2 from memory and an Ecol array"); return -1; }
        const int CCl = (C > 256 && C % 256 == 0 && C / 256 <= ECA_MAX_CHUNKS) ? 256 : C, nchunkl = C / CCl;
        hipLaunchKernelGGL(eca_bwd_sample_kernel, dim3(B, nchunkl), dim3(256), (size_t)(2 * (CCl + 4) + 2 * (CCl + 16)) * sizeof(float), s, S1, S2, gn, sgate, w5, gamma, beta, E, dw5part, C, CCl, PsaStats{});
        hipLaunchKernelGGL(eca_bn_bwd_channel_len_kernel, dim3((C + FIN_CL - 1) / FIN_CL), dim3(FIN_CL * FIN_BL), 0, s, S1, S2, gap, sgate, mean, rstd, dgamma, dbeta, E, Ecol, Fc,
                           dw5part, B * nchunkl, dw5, frame_len, B, T, C);
        return launch_rc();
    }
    PsaStats p = ps ? *ps : PsaStats{};
    if (p.G && (C % 8 != 0 || p.ldt % 8 != 0 || ((uintptr_t)p.Wt) % 16 != 0)) { ishara_set_error("eca_bn_bwd_finalize: PsaStats needs C %% 8 == 0 and 16-byte aligned weight rows"); return -1; }
    const int CC = (C > 256 && C % 256 == 0 && C / 256 <= ECA_MAX_CHUNKS) ? 256 : C, nchunk = C / CC;      // dw5part: B * nchunk * 8 floats
    const size_t shm = (size_t)(2 * (CC + 4) + 2 * (CC + 16) + (p.G ? p.N + 4 * (CC + 16) : 0)) * sizeof(float);
    hipLaunchKernelGGL(eca_bwd_sample_kernel, dim3(B, nchunk), dim3(256), shm, s, S1, S2, gn, sgate, w5, gamma, beta, E, dw5part, C, CC, p);
    hipLaunchKernelGGL(eca_bn_bwd_channel_kernel, dim3((C + FIN_CL - 1) / FIN_CL), dim3(FIN_CL * FIN_BL), 0, s, S1, S2, gap, sgate, mean, rstd, dgamma, dbeta, E, Fc, dw5part, B * nchunk, dw5, B, T, C);
    return launch_rc();
}

__global__ __launch_bounds__(1024) void bn_bwd_channel_kernel(const float* __restrict__ S1, const float* __restrict__ S2, float* __restrict__ dgamma,
                                      float* __restrict__ dbeta, float* __restrict__ Ecol, float* __restrict__ Fc, int B, int Tn, int C) {
    __shared__ double rg_[FIN_NW][FIN_CL], rb_[FIN_NW][FIN_CL];
    const int cl = threadIdx.x & (FIN_CL - 1), bl = threadIdx.x / FIN_CL, wv = threadIdx.x >> 6;
    const int c = blockIdx.x * FIN_CL + cl;
    double dg = 0.0, db = 0.0;
    if (c < C)
        for (int b = bl; b < B; b += FIN_BL) { dg += (double)S2[(size_t)b * C + c]; db += (double)S1[(size_t)b * C + c]; }
    dg = fin_fold(dg); db = fin_fold(db);
    if ((threadIdx.x & 63) < FIN_CL) { rg_[wv][cl] = dg; rb_[wv][cl] = db; }
    __syncthreads();
    if (bl != 0 || c >= C) return;
    for (int i = 1; i < FIN_NW; ++i) { dg += rg_[i][cl]; db += rb_[i][cl]; }
    const float mtot = (float)B * (float)Tn;
    dgamma[c] += (float)dg;
    dbeta[c] += (float)db;
    Fc[c] = (float)dg / mtot;
    Ecol[c] = -(float)db / mtot;
}

int launch_bn_bwd_finalize(const float* S1, const float* S2, float* dgamma, float* dbeta, float* Ecol, float* Fc,
                           int B, int T, int C, hipStream_t s) {
    hipLaunchKernelGGL(bn_bwd_channel_kernel, dim3((C + FIN_CL - 1) / FIN_CL), dim3(FIN_CL * FIN_BL), 0, s, S1, S2, dgamma, dbeta, Ecol, Fc, B, T, C);
    return launch_rc();
}

// dx = a[c] * (dy*sg[b,c] + E - xhat*Fc[c]) = dy*k1 + k0 - x*k2 with per-(sample,channel) constants
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, const float* __restrict__ a, const float* __restrict__ sg,
                                                           const float* __restrict__ E, int e_per_sample, const float* __restrict__ Fc,
                                                           T* __restrict__ dx, int Tn, int C) {
    const int nch = C >> 3;
    const int cpr = min(nch, 256), rpb = 256 / cpr;
    const int cl = threadIdx.x % cpr, rl = threadIdx.x / cpr;
    const int b = blockIdx.y;
    if (rl >= rpb) return;
    for (int chunk = cl; chunk < nch; chunk += cpr) {
        const int ch = chunk * 8;
        float k0[8], k1[8], k2[8];
        {
            float mu[8], rs[8], aa[8], fc[8], ee[8], g[8];
            load8(mean + ch, mu); load8(rstd + ch, rs); load8(a + ch, aa); load8(Fc + ch, fc);
            load8(E + (e_per_sample ? (size_t)b * C : 0) + ch, ee);
            if (sg) load8(sg + (size_t)b * C + ch, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                k2[e] = aa[e] * rs[e] * fc[e];
                k1[e] = aa[e] * (sg ? g[e] : 1.f);
                k0[e] = aa[e] * ee[e] + mu[e] * k2[e];
            }
        }
        for (int t = blockIdx.x * rpb + rl; t < Tn; t += gridDim.x * rpb) {
            const size_t off = ((size_t)b * Tn + t) * C + ch;
            float d[8], xv[8];
            load8(dy + off, d);
            load8(x + off, xv);
#pragma unroll
            for (int e = 0; e < 8; ++e) d[e] = d[e] * k1[e] + k0[e] - xv[e] * k2[e];
            store8(dx + off, d);
        }
    }
}

int launch_bn_bwd_apply(int dt, const void* dy, const void* x, const float* mean, const float* rstd, const float* a,
                        const float* sg, const float* E, int e_per_sample, const float* Fc, void* dx,
                        int B, int T, int C, hipStream_t s) {
    if (C % 8 != 0) { ishara_set_error("bn_bwd_apply: C%%8 != 0"); return -1; }
    const int cpr = min(C / 8, 256), rpb = 256 / cpr;
    int gx = (T + rpb - 1) / rpb;
    const int cap = max(1, 4096 / max(B, 1));
    if (gx > cap) gx = cap;
    dim3 grid(gx, B);
    if (dt == DT_BF16) hipLaunchKernelGGL(bn_bwd_apply_kernel<bf16>, grid, dim3(256), 0, s, (const bf16*)dy, (const bf16*)x, mean, rstd, a, sg, E, e_per_sample, Fc, (bf16*)dx, T, C);
    else hipLaunchKernelGGL(bn_bwd_apply_kernel<float>, grid, dim3(256), 0, s, (const float*)dy, (const float*)x, mean, rstd, a, sg, E, e_per_sample, Fc, (float*)dx, T, C);
    return launch_rc();
}

// =====================================================================================
// Squeeze-Excite MLP (one workgroup per sample; C <= 1024, R <= 128)
// =====================================================================================
// sum_i v[i0 + i * vstep] * w[i * wstride] over n terms, 16 weight loads in flight (these matvecs are chains of L2 latencies, not of bytes)
DEVI float se_dot(const float* __restrict__ w, size_t wstride, const float* v, int vstep, int n) {
    float acc = 0.f;
    int i = 0;
    for (; i + 16 <= n; i += 16) {
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) t[u] = w[(size_t)(i + u) * wstride];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc += t[u] * v[(i + u) * vstep];
    }
    for (; i < n; ++i) acc += w[(size_t)i * wstride] * v[i * vstep];
    return acc;
}
__global__ __launch_bounds__(256) void se_fwd_kernel(const float* __restrict__ gap, float invT, const float* __restrict__ W1, const float* __restrict__ b1,
                                                     const float* __restrict__ W2, const float* __restrict__ b2, float* __restrict__ hid_pre,
                                                     float* __restrict__ se, int C, int R) {
    extern __shared__ float sh[];   // z[C], h[R], part[256]
    float* z = sh;
    float* h = sh + C;
    float* part = h + R;
    const int b = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += blockDim.x) z[c] = gap[(size_t)b * C + c] * invT;
    __syncthreads();
    if (R <= 256 && 256 % R == 0 && blockDim.x == 256) {      // the squeeze matvec over all 256 threads: thread (r, p) sums every (256 / R)-th channel
        const int np = 256 / R, r = threadIdx.x % R, p = threadIdx.x / R;      // (R threads over all C channels: a 65 us chain of loads at C = 512)
        part[p * R + r] = se_dot(W1 + (size_t)p * R + r, (size_t)np * R, z + p, np, (C - p + np - 1) / np);
        __syncthreads();
        if (threadIdx.x < R) {
            float t = b1[r];
            for (int q = 0; q < np; ++q) t += part[q * R + r];
            hid_pre[(size_t)b * R + r] = t;
            h[r] = swishf_(t);
        }
    } else {
        for (int r = threadIdx.x; r < R; r += blockDim.x) {
            float acc = b1[r];
            for (int c = 0; c < C; ++c) acc += z[c] * W1[(size_t)c * R + r];
            hid_pre[(size_t)b * R + r] = acc;
            h[r] = swishf_(acc);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) se[(size_t)b * C + c] = sigmoidf_(b2[c] + se_dot(W2 + c, (size_t)C, h, 1, R));
}

int launch_se_fwd(const float* gap, float invT, const float* W1, const float* b1, const float* W2, const float* b2,
                  float* hid_pre, float* se, int B, int C, int R, hipStream_t s) {
    hipLaunchKernelGGL(se_fwd_kernel, dim3(B), dim3(256), (C + R + 256) * sizeof(float), s, gap, invT, W1, b1, W2, b2, hid_pre, se, C, R);
    return launch_rc();
}

// Squeeze-excite backward, step 1 (one workgroup per sample): dz2 = dse*se*(1-se), dhp = (W2 dz2) * swish'(hid_pre), dgapT = W1 dhp / T;
// dz2, dhp and h = swish(hid_pre) go to scr[b][C + 2R] for the weight-gradient pass
__global__ __launch_bounds__(256) void se_bwd_kernel(const float* __restrict__ dse, const float* __restrict__ gap, float invT,
                                                     const float* __restrict__ W1, const float* __restrict__ W2,
                                                     const float* __restrict__ hid_pre, const float* __restrict__ se,
                                                     float* __restrict__ scr, float* __restrict__ dgapT, int C, int R) {
    extern __shared__ float sh[];   // dp2[C], dhp[R], part[256]
    float* dp2 = sh;
    float* dhp = sh + C;
    float* part = dhp + R;
    const int b = blockIdx.x;
    float* sb = scr + (size_t)b * (C + 2 * R);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        const size_t i = (size_t)b * C + c;
        const float sv = se[i];
        const float d = dse[i] * sv * (1.f - sv);
        dp2[c] = d;
        sb[c] = d;
    }
    __syncthreads();
    if (R <= 256 && 256 % R == 0 && blockDim.x == 256) {      // W2[r, :] . dp2 over all 256 threads: thread (p, r) takes the channels c = p mod (256 / R)
        const int np = 256 / R, r = threadIdx.x / np, p = threadIdx.x % np;      // consecutive threads read consecutive channels of one weight row
        part[r * np + p] = se_dot(W2 + (size_t)r * C + p, (size_t)np, dp2 + p, np, (C - p + np - 1) / np);
        __syncthreads();
        if (threadIdx.x < R) {
            const int rr = threadIdx.x;
            float t = 0.f;
            for (int q = 0; q < np; ++q) t += part[rr * np + q];
            const float hp = hid_pre[(size_t)b * R + rr];
            const float d = t * dswishf_(hp);
            dhp[rr] = d;
            sb[C + rr] = d;
            sb[C + R + rr] = swishf_(hp);
        }
    } else {
        for (int r = threadIdx.x; r < R; r += blockDim.x) {
            float acc = 0.f;
            for (int c = 0; c < C; ++c) acc += W2[(size_t)r * C + c] * dp2[c];
            const float hp = hid_pre[(size_t)b * R + r];
            const float d = acc * dswishf_(hp);
            dhp[r] = d;
            sb[C + r] = d;
            sb[C + R + r] = swishf_(hp);
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += blockDim.x) dgapT[(size_t)b * C + c] = se_dot(W1 + (size_t)c * R, 1, dhp, 1, R) * invT;
}
// step 2: weight gradients as sums over the samples in a fixed order (no float atomics: the gradients repeat bit for bit).
// workgroup = 64 parameters (lane) x 4 sample groups (wave w takes b = w, w+4, ...; 8 independent loads in flight), combined through LDS:
// dW1[c][r] += sum_b z[b,c]*dhp[b,r], db1[r] += sum_b dhp[b,r], dW2[r][c] += sum_b h[b,r]*dz2[b,c], db2[c] += sum_b dz2[b,c]
__global__ __launch_bounds__(256) void se_wgrad_kernel(const float* __restrict__ scr, const float* __restrict__ gap, float invT,
                                                       float* __restrict__ dW1, float* __restrict__ db1, float* __restrict__ dW2, float* __restrict__ db2,
                                                       int B, int C, int R) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + lane;
    const int CR = C * R, S = C + 2 * R;
    // parameter i -> (first factor pointer / stride, second factor pointer / stride, output)
    const float* f0 = nullptr; const float* f1 = nullptr; size_t s0 = 0, s1 = S; float sc = 1.f; float* out = nullptr;
    if (i < CR) { const int r = i / C, c = i - r * C; f0 = scr + C + R + r; s0 = S; f1 = scr + c; out = dW2 + i; }                       // dW2[r][c]: c fastest
    else if (i < 2 * CR) { const int k = i - CR, c = k / R, r = k - c * R; f0 = gap + c; s0 = C; sc = invT; f1 = scr + C + r; out = dW1 + k; }   // dW1[c][r]
    else if (i < 2 * CR + C) { f1 = scr + (i - 2 * CR); out = db2 + (i - 2 * CR); }
    else if (i < 2 * CR + C + R) { f1 = scr + C + (i - 2 * CR - C); out = db1 + (i - 2 * CR - C); }
    float acc = 0.f;
    if (out) {
        for (int b0 = w; b0 < B; b0 += 32) {
            float a[8], c8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int b = b0 + 4 * u;
                a[u] = (b < B && f0) ? f0[(size_t)b * s0] : 1.f;
                c8[u] = b < B ? f1[(size_t)b * s1] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += a[u] * sc * c8[u];
        }
    }
    red[w][lane] = acc;
    __syncthreads();
    if (w == 0 && out) *out += red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
}

// scr: B * (C + 2R) floats of scratch
int launch_se_bwd(const float* dse, const float* gap, float invT, const float* W1, const float* W2,
                  const float* hid_pre, const float* se, float* dW1, float* db1, float* dW2, float* db2,
                  float* dgapT, float* scr, int B, int C, int R, hipStream_t s) {
    hipLaunchKernelGGL(se_bwd_kernel, dim3(B), dim3(256), (C + R + 256) * sizeof(float), s, dse, gap, invT, W1, W2, hid_pre, se, scr, dgapT, C, R);
    hipLaunchKernelGGL(se_wgrad_kernel, dim3((2 * C * R + C + R + 63) / 64), dim3(256), 0, s, scr, gap, invT, dW1, db1, dW2, db2, B, C, R);
    return launch_rc();
}
