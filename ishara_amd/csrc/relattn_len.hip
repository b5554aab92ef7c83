// The fp32 lane kernels of the torch Squeezeformer family's relative-position attention (RelativeMultiHeadAttention.forward, attention.py:75-92),
// forward and three backward passes: one thread per query (forward, dq) / key (dk, dv) / table row (dpos), the other side streamed through LDS
// in chunks, no [T, T] matrix in memory; the backward passes recompute the probabilities from the saved log-sum-exp.
//   q, k, v [B*T, d] (head h in columns h*DH ..), posp [2T-1, d] f32 (pos_proj of the table), u, vb [d] f32.
//   score(i,j) = scale * ((q_i+u).k_j + (q_i+vb).posp[T-1-i+j]) (`_relative_shift`, attention.py:102-110, in closed form); softmax over j;
//   inverted dropout on the probabilities (row key (b*H+h)*T+i, column = key, 8-bit threshold).
// PER-CLIP KEY LENGTHS (the padding mask in its (batch, 1, time2) form): the keys j >= n[b] of clip b are masked for every query and head,
// n[b] = clamp(key_len[b], 0, T); a null key_len means every key, n[b] = T (attn_key_count, kernels.h): the call without lengths runs these same
// kernels.  The reference fills the masked scores with -1e9; in fp32 exp underflows to exactly 0 for a clip with at least one valid key, so the
// kernels SKIP the keys instead: every key loop sweeps ceil(n[b] / RL_KT) chunks only and no K / V row at or past n[b] is read into a sum (they
// are staged as zero).  Query rows past n[b] are computed like any other: only keys are masked.
//   n[b] = 0 (a dead clip): o = 0, lse = ATT_DEAD_LSE, dq = 0, and its dO reaches neither dk / dv nor du / dvb / dposp.  The reference's fill
//   would average the padding uniformly there; zeros are this library's convention ("Fully masked rows").
//   Every output is overwritten: the dk / dv rows of the keys >= n[b] are exact zeros (a workgroup holding only such keys sweeps nothing).
// du / dvb / dposp are fp32 atomics into buffers the caller has zero-filled.
// Which kernels a call runs is stated once, by relattn_route below; the MFMA forward of the masked bf16 call is relattn_mfma.hip.
#include "model_types.h"

#define RL_QB 64      // threads per workgroup = queries / keys / table rows per workgroup
#define RL_KT 32      // rows of the streamed side per chunk

template <typename T> DEVI float rl_ldf(const T* p) { return to_f(*p); }

// ------------------------------------------------------------------ forward
template <typename T, int DH>
__global__ __launch_bounds__(RL_QB) void relattn_len_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const float* __restrict__ posp,
                                                                const float* __restrict__ u, const float* __restrict__ vb, T* __restrict__ o, float* __restrict__ lse,
                                                                const int* __restrict__ key_len, int H, int Tn, float scale, DropSpec drop) {
    __shared__ float Ks[RL_KT][DH + 1], Vs[RL_KT][DH + 1], Ps[RL_KT + RL_QB - 1][DH + 1];
    const int d = H * DH, bh = blockIdx.y, b = bh / H, h = bh % H, i0 = blockIdx.x * RL_QB, i = i0 + threadIdx.x;
    const bool act = i < Tn;
    const int n = attn_key_count(key_len, b, Tn);
    float qu[DH], qv[DH], acc[DH];
    {
        const T* qp = q + ((size_t)b * Tn + (act ? i : 0)) * d + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) { const float x = rl_ldf(qp + e); qu[e] = x + u[h * DH + e]; qv[e] = x + vb[h * DH + e]; acc[e] = 0.f; }
    }
    float mx = -3.0e38f, l = 0.f;
    const uint32_t rk = rng_row_key(drop.key, (uint32_t)(bh * Tn + i));
    for (int j0 = 0; j0 < n; j0 += RL_KT) {
        const int rbase = Tn - 1 - (i0 + RL_QB - 1) + j0;
        __syncthreads();
        for (int x = threadIdx.x; x < RL_KT * DH; x += RL_QB) {
            const int jj = x / DH, e = x % DH, j = j0 + jj;
            Ks[jj][e] = j < n ? rl_ldf(k + ((size_t)b * Tn + j) * d + h * DH + e) : 0.f;
            Vs[jj][e] = j < n ? rl_ldf(v + ((size_t)b * Tn + j) * d + h * DH + e) : 0.f;
        }
        for (int x = threadIdx.x; x < (RL_KT + RL_QB - 1) * DH; x += RL_QB) {
            const int rr = x / DH, e = x % DH, r = rbase + rr;
            Ps[rr][e] = (r >= 0 && r < 2 * Tn - 1) ? posp[(size_t)r * d + h * DH + e] : 0.f;
        }
        __syncthreads();
        if (!act) continue;
        const int pr0 = i0 + RL_QB - 1 - i;
        for (int jj = 0; jj < RL_KT && j0 + jj < n; ++jj) {
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < DH; ++e) s += qu[e] * Ks[jj][e] + qv[e] * Ps[pr0 + jj][e];
            s *= scale;
            const float mn = fmaxf(mx, s), corr = __expf(mx - mn), p = __expf(s - mn);
            l = l * corr + p;
            const float pd = (drop.thr == 0u || rng_keep_q(rk, (uint32_t)(j0 + jj), drop.thr)) ? p * drop.scale : 0.f;
#pragma unroll
            for (int e = 0; e < DH; ++e) acc[e] = acc[e] * corr + pd * Vs[jj][e];
            mx = mn;
        }
    }
    if (act) {
        const bool dead = n == 0;                 // no key: the clip is all padding at this resolution
        const float inv = dead ? 0.f : 1.f / l;
        T* op = o + ((size_t)b * Tn + i) * d + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) op[e] = from_f<T>(acc[e] * inv);
        lse[(size_t)bh * Tn + i] = dead ? ATT_DEAD_LSE : mx + __logf(l);
    }
}

// ------------------------------------------------------------------ dq, delta, du / dvb
template <typename T, int DH>
__global__ __launch_bounds__(RL_QB) void relattn_len_bwd_dq_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const float* __restrict__ posp,
                                                                   const float* __restrict__ u, const float* __restrict__ vb, const T* __restrict__ o, const T* __restrict__ dO,
                                                                   const float* __restrict__ lse, float* __restrict__ delta, T* __restrict__ dq,
                                                                   float* __restrict__ du, float* __restrict__ dvb, const int* __restrict__ key_len,
                                                                   int H, int Tn, float scale, DropSpec drop) {
    __shared__ float Ks[RL_KT][DH + 1], Vs[RL_KT][DH + 1], Ps[RL_KT + RL_QB - 1][DH + 1];
    const int d = H * DH, bh = blockIdx.y, b = bh / H, h = bh % H, i0 = blockIdx.x * RL_QB, i = i0 + threadIdx.x;
    const bool act = i < Tn;
    const int n = attn_key_count(key_len, b, Tn);
    float qu[DH], qv[DH], go[DH], dqc[DH], dqp[DH];
    float D = 0.f, L = 0.f;
    {
        const size_t row = ((size_t)b * Tn + (act ? i : 0)) * d + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) {
            const float x = rl_ldf(q + row + e);
            qu[e] = x + u[h * DH + e]; qv[e] = x + vb[h * DH + e];
            go[e] = act ? rl_ldf(dO + row + e) : 0.f;
            D += go[e] * rl_ldf(o + row + e);
            dqc[e] = 0.f; dqp[e] = 0.f;
        }
        if (act) { L = lse[(size_t)bh * Tn + i]; delta[(size_t)bh * Tn + i] = D; }
    }
    const uint32_t rk = rng_row_key(drop.key, (uint32_t)(bh * Tn + i));
    for (int j0 = 0; j0 < n; j0 += RL_KT) {
        const int rbase = Tn - 1 - (i0 + RL_QB - 1) + j0;
        __syncthreads();
        for (int x = threadIdx.x; x < RL_KT * DH; x += RL_QB) {
            const int jj = x / DH, e = x % DH, j = j0 + jj;
            Ks[jj][e] = j < n ? rl_ldf(k + ((size_t)b * Tn + j) * d + h * DH + e) : 0.f;
            Vs[jj][e] = j < n ? rl_ldf(v + ((size_t)b * Tn + j) * d + h * DH + e) : 0.f;
        }
        for (int x = threadIdx.x; x < (RL_KT + RL_QB - 1) * DH; x += RL_QB) {
            const int rr = x / DH, e = x % DH, r = rbase + rr;
            Ps[rr][e] = (r >= 0 && r < 2 * Tn - 1) ? posp[(size_t)r * d + h * DH + e] : 0.f;
        }
        __syncthreads();
        if (!act) continue;
        const int pr0 = i0 + RL_QB - 1 - i;
        for (int jj = 0; jj < RL_KT && j0 + jj < n; ++jj) {
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int e = 0; e < DH; ++e) { s += qu[e] * Ks[jj][e] + qv[e] * Ps[pr0 + jj][e]; dp += go[e] * Vs[jj][e]; }
            const float p = __expf(s * scale - L);
            if (!(drop.thr == 0u || rng_keep_q(rk, (uint32_t)(j0 + jj), drop.thr))) dp = 0.f; else dp *= drop.scale;
            const float dS = p * (dp - D) * scale;
#pragma unroll
            for (int e = 0; e < DH; ++e) { dqc[e] += dS * Ks[jj][e]; dqp[e] += dS * Ps[pr0 + jj][e]; }
        }
    }
    if (act) {
        T* dp_ = dq + ((size_t)b * Tn + i) * d + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) dp_[e] = from_f<T>(dqc[e] + dqp[e]);
    }
    if (n == 0) return;      // uniform over the workgroup: a dead clip adds nothing to du / dvb
    // u_bias gradient = sum over queries of the content part, v_bias gradient = of the positional part
    __syncthreads();
    float (*red)[DH + 1] = Ps;       // RL_QB rows available
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int e = 0; e < DH; ++e) red[threadIdx.x][e] = act ? (pass == 0 ? dqc[e] : dqp[e]) : 0.f;
        __syncthreads();
        for (int e = threadIdx.x; e < DH; e += RL_QB) {
            float s = 0.f;
            for (int t = 0; t < RL_QB; ++t) s += red[t][e];
            atomicAdd(&(pass == 0 ? du : dvb)[h * DH + e], s);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ dk, dv: one thread per key, queries streamed
template <typename T, int DH>
__global__ __launch_bounds__(RL_QB) void relattn_len_bwd_dkv_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const float* __restrict__ posp,
                                                                    const float* __restrict__ u, const float* __restrict__ vb, const T* __restrict__ dO,
                                                                    const float* __restrict__ lse, const float* __restrict__ delta, T* __restrict__ dk, T* __restrict__ dv,
                                                                    const int* __restrict__ key_len, int H, int Tn, float scale, DropSpec drop) {
    __shared__ float Qs[RL_KT][DH + 1], Gs[RL_KT][DH + 1], Ps[RL_KT + RL_QB - 1][DH + 1], Ls[RL_KT], Ds[RL_KT];
    const int d = H * DH, bh = blockIdx.y, b = bh / H, h = bh % H, j0 = blockIdx.x * RL_QB, j = j0 + threadIdx.x;
    const bool act = j < Tn;
    const int n = attn_key_count(key_len, b, Tn);
    const bool kin = j < n;                      // n <= T
    float kk[DH], vv[DH], ak[DH], av[DH], uu[DH], vbv[DH];
    float uk = 0.f;
    {
        const size_t row = ((size_t)b * Tn + (kin ? j : 0)) * d + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) {
            kk[e] = rl_ldf(k + row + e); vv[e] = rl_ldf(v + row + e); ak[e] = 0.f; av[e] = 0.f;
            uu[e] = u[h * DH + e]; vbv[e] = vb[h * DH + e];
            uk += uu[e] * kk[e];
        }
    }
    const int nq = j0 < n ? Tn : 0;              // uniform: a workgroup whose keys all lie past n[b] sweeps nothing and writes zeros
    for (int i0 = 0; i0 < nq; i0 += RL_KT) {
        // rows of the table this chunk needs: r = T-1-i+j for i in [i0, i0+KT), j in [j0, j0+QB): from T-1-(i0+KT-1)+j0
        const int rbase = Tn - 1 - (i0 + RL_KT - 1) + j0;
        __syncthreads();
        for (int x = threadIdx.x; x < RL_KT * DH; x += RL_QB) {
            const int ii = x / DH, e = x % DH, i = i0 + ii;
            Qs[ii][e] = i < Tn ? rl_ldf(q + ((size_t)b * Tn + i) * d + h * DH + e) : 0.f;
            Gs[ii][e] = i < Tn ? rl_ldf(dO + ((size_t)b * Tn + i) * d + h * DH + e) : 0.f;
        }
        for (int x = threadIdx.x; x < RL_KT; x += RL_QB) { const int i = i0 + x; Ls[x] = i < Tn ? lse[(size_t)bh * Tn + i] : 0.f; Ds[x] = i < Tn ? delta[(size_t)bh * Tn + i] : 0.f; }
        for (int x = threadIdx.x; x < (RL_KT + RL_QB - 1) * DH; x += RL_QB) {
            const int rr = x / DH, e = x % DH, r = rbase + rr;
            Ps[rr][e] = (r >= 0 && r < 2 * Tn - 1) ? posp[(size_t)r * d + h * DH + e] : 0.f;
        }
        __syncthreads();
        if (!kin) continue;
        for (int ii = 0; ii < RL_KT && i0 + ii < Tn; ++ii) {
            const int pr = (RL_KT - 1 - ii) + (int)threadIdx.x;          // (T-1-(i0+ii)+j) - rbase
            float s = uk, dp = 0.f;
#pragma unroll
            for (int e = 0; e < DH; ++e) { s += Qs[ii][e] * kk[e] + (Qs[ii][e] + vbv[e]) * Ps[pr][e]; dp += Gs[ii][e] * vv[e]; }
            const float p = __expf(s * scale - Ls[ii]);
            const bool keep = drop.thr == 0u || rng_keep_q(rng_row_key(drop.key, (uint32_t)(bh * Tn + i0 + ii)), (uint32_t)j, drop.thr);
            const float pd = keep ? p * drop.scale : 0.f;
            dp = keep ? dp * drop.scale : 0.f;
            const float dS = p * (dp - Ds[ii]) * scale;
#pragma unroll
            for (int e = 0; e < DH; ++e) { ak[e] += dS * (Qs[ii][e] + uu[e]); av[e] += pd * Gs[ii][e]; }
        }
    }
    if (act) {      // a key at or past n[b] never entered the loop: ak = av = 0 exactly
        const size_t row = ((size_t)b * Tn + j) * d + h * DH;
#pragma unroll
        for (int e = 0; e < DH; ++e) { dk[row + e] = from_f<T>(ak[e]); dv[row + e] = from_f<T>(av[e]); }
    }
}

// ------------------------------------------------------------------ dposp: one thread per table row, the (i, j) pairs with T-1-i+j == r and j < n[b]
// A length-aware fp32 gather kernel (there is no MFMA dposp yet)
template <typename T, int DH>
__global__ __launch_bounds__(RL_QB) void relattn_len_bwd_dpos_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const float* __restrict__ posp,
                                                                     const float* __restrict__ u, const float* __restrict__ vb, const T* __restrict__ dO,
                                                                     const float* __restrict__ lse, const float* __restrict__ delta, float* __restrict__ dposp,
                                                                     const int* __restrict__ key_len, int H, int Tn, float scale, DropSpec drop) {
    __shared__ float Qs[RL_KT][DH + 1], Gs[RL_KT][DH + 1], Ks[RL_KT + RL_QB - 1][DH + 1], Vs[RL_KT + RL_QB - 1][DH + 1], Ls[RL_KT], Ds[RL_KT];
    const int d = H * DH, bh = blockIdx.y, b = bh / H, h = bh % H, r0 = blockIdx.x * RL_QB, r = r0 + threadIdx.x;
    const bool act = r < 2 * Tn - 1;
    const int n = attn_key_count(key_len, b, Tn);
    // the keys of this workgroup's rows: j = i + r - (T-1) >= r0 - (T-1); none below n[b]: nothing to add (uniform)
    if (r0 - (Tn - 1) >= n) return;
    float pp[DH], acc[DH], uu[DH], vbv[DH];
#pragma unroll
    for (int e = 0; e < DH; ++e) { pp[e] = act ? posp[(size_t)r * d + h * DH + e] : 0.f; acc[e] = 0.f; uu[e] = u[h * DH + e]; vbv[e] = vb[h * DH + e]; }
    for (int i0 = 0; i0 < Tn; i0 += RL_KT) {
        // keys: j = i + r - (T-1) for i in [i0, i0+KT), r in [r0, r0+QB): from jbase = i0 + r0 - (T-1)
        const int jbase = i0 + r0 - (Tn - 1);
        if (jbase >= n) break;                   // uniform; jbase grows with i0
        __syncthreads();
        for (int x = threadIdx.x; x < RL_KT * DH; x += RL_QB) {
            const int ii = x / DH, e = x % DH, i = i0 + ii;
            Qs[ii][e] = i < Tn ? rl_ldf(q + ((size_t)b * Tn + i) * d + h * DH + e) : 0.f;
            Gs[ii][e] = i < Tn ? rl_ldf(dO + ((size_t)b * Tn + i) * d + h * DH + e) : 0.f;
        }
        for (int x = threadIdx.x; x < RL_KT; x += RL_QB) { const int i = i0 + x; Ls[x] = i < Tn ? lse[(size_t)bh * Tn + i] : 0.f; Ds[x] = i < Tn ? delta[(size_t)bh * Tn + i] : 0.f; }
        for (int x = threadIdx.x; x < (RL_KT + RL_QB - 1) * DH; x += RL_QB) {
            const int jj = x / DH, e = x % DH, j = jbase + jj;
            const bool ok = j >= 0 && j < n;
            Ks[jj][e] = ok ? rl_ldf(k + ((size_t)b * Tn + j) * d + h * DH + e) : 0.f;
            Vs[jj][e] = ok ? rl_ldf(v + ((size_t)b * Tn + j) * d + h * DH + e) : 0.f;
        }
        __syncthreads();
        if (!act) continue;
        for (int ii = 0; ii < RL_KT && i0 + ii < Tn; ++ii) {
            const int jl = ii + (int)threadIdx.x, j = jbase + jl;
            if (j < 0 || j >= n) continue;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int e = 0; e < DH; ++e) { s += (Qs[ii][e] + uu[e]) * Ks[jl][e] + (Qs[ii][e] + vbv[e]) * pp[e]; dp += Gs[ii][e] * Vs[jl][e]; }
            const float p = __expf(s * scale - Ls[ii]);
            const bool keep = drop.thr == 0u || rng_keep_q(rng_row_key(drop.key, (uint32_t)(bh * Tn + i0 + ii)), (uint32_t)j, drop.thr);
            dp = keep ? dp * drop.scale : 0.f;
            const float dS = p * (dp - Ds[ii]) * scale;
#pragma unroll
            for (int e = 0; e < DH; ++e) acc[e] += dS * (Qs[ii][e] + vbv[e]);
        }
    }
    if (act) {
#pragma unroll
        for (int e = 0; e < DH; ++e) atomicAdd(&dposp[(size_t)r * d + h * DH + e], acc[e]);
    }
}

// ------------------------------------------------------------------ the route, stated once
// masked = per-clip key lengths given.  The masked bf16 call at head dim 32 / 64 runs the MFMA forward of relattn_mfma.hip and the lane backward
// above; everything else the family has (the call without lengths at any dtype and head dim, f32, bf16 at dh 8 / 16, any T >= 1) runs the lane
// kernels, forward too.  MFMA dq / dkv / dposp: DESIGN.md §8
RelAttnRoute relattn_route(int dt, int T, int dh, bool masked) {
    RelAttnRoute r;
    if (dt != DT_F32 && dt != DT_BF16) { r.kind = RELATTN_REFUSED; r.why = "relative attention: f32 / bf16 only"; return r; }
    if (!relattn_head_dim_ok(dh)) { r.kind = RELATTN_REFUSED; r.why = "relative attention: head dim unsupported (" RELATTN_HEAD_DIMS ")"; return r; }
    if (T < 1) { r.kind = RELATTN_REFUSED; r.why = "relative attention: T must be >= 1"; return r; }
    r.kind = (masked && dt == DT_BF16 && (dh == 32 || dh == 64)) ? RELATTN_MFMA_LEN : RELATTN_LANE;
    return r;
}
const char* relattn_kernel_name(const RelAttnRoute& r, bool backward) {
    if (r.kind != RELATTN_LANE && r.kind != RELATTN_MFMA_LEN) return "";
    if (backward) return "relattn_len_bwd_dq_kernel+relattn_len_bwd_dkv_kernel+relattn_len_bwd_dpos_kernel";
    return r.kind == RELATTN_MFMA_LEN ? "relattn_len_fwd_mfma_kernel" : "relattn_len_fwd_kernel";
}

#define RL_DISPATCH(KERNEL, TT, grid, s, ...)                                                                           \
    switch (dh) {                                                                                                       \
        case 8: hipLaunchKernelGGL((KERNEL<TT, 8>), grid, dim3(RL_QB), 0, s, __VA_ARGS__); break;                        \
        case 16: hipLaunchKernelGGL((KERNEL<TT, 16>), grid, dim3(RL_QB), 0, s, __VA_ARGS__); break;                      \
        case 32: hipLaunchKernelGGL((KERNEL<TT, 32>), grid, dim3(RL_QB), 0, s, __VA_ARGS__); break;                      \
        case 64: hipLaunchKernelGGL((KERNEL<TT, 64>), grid, dim3(RL_QB), 0, s, __VA_ARGS__); break;                      \
        default: ishara_set_error("relative attention: head dim %d unsupported (" RELATTN_HEAD_DIMS ")", dh); return -1; \
    }

// key_len NULL: every key.  force_lane: the operator entry points' `route` = 1, the lane kernels where the route would choose the MFMA forward
int launch_relattn_len_fwd(int dt, const void* q, const void* k, const void* v, const float* posp, const float* u, const float* vb, void* o, float* lse,
                           const int* key_len, bool force_lane, int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s) {
    const RelAttnRoute r = relattn_route(dt, T, dh, key_len != nullptr);
    if (r.kind == RELATTN_REFUSED) { ishara_set_error("%s", r.why); return -1; }
    if (r.kind == RELATTN_MFMA_LEN && !force_lane) return launch_relattn_len_fwd_mfma(q, k, v, posp, u, vb, o, lse, key_len, B, H, T, dh, scale, drop, s);
    const dim3 grid((T + RL_QB - 1) / RL_QB, B * H);
    if (dt == DT_BF16) { RL_DISPATCH(relattn_len_fwd_kernel, bf16, grid, s, (const bf16*)q, (const bf16*)k, (const bf16*)v, posp, u, vb, (bf16*)o, lse, key_len, H, T, scale, drop) }
    else { RL_DISPATCH(relattn_len_fwd_kernel, float, grid, s, (const float*)q, (const float*)k, (const float*)v, posp, u, vb, (float*)o, lse, key_len, H, T, scale, drop) }
    return launch_rc();
}
// one backward for every route: the lane kernels
int launch_relattn_len_bwd(int dt, const void* q, const void* k, const void* v, const float* posp, const float* u, const float* vb, const void* o, const void* dO,
                           const float* lse, float* delta, void* dq, void* dk, void* dv, float* du, float* dvb, float* dposp,
                           const int* key_len, int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s) {
    const RelAttnRoute r = relattn_route(dt, T, dh, key_len != nullptr);
    if (r.kind == RELATTN_REFUSED) { ishara_set_error("%s", r.why); return -1; }
    const dim3 gq((T + RL_QB - 1) / RL_QB, B * H), gp((2 * T - 1 + RL_QB - 1) / RL_QB, B * H);
    if (dt == DT_BF16) {
        RL_DISPATCH(relattn_len_bwd_dq_kernel, bf16, gq, s, (const bf16*)q, (const bf16*)k, (const bf16*)v, posp, u, vb, (const bf16*)o, (const bf16*)dO, lse, delta, (bf16*)dq, du, dvb, key_len, H, T, scale, drop)
        RL_DISPATCH(relattn_len_bwd_dkv_kernel, bf16, gq, s, (const bf16*)q, (const bf16*)k, (const bf16*)v, posp, u, vb, (const bf16*)dO, lse, (const float*)delta, (bf16*)dk, (bf16*)dv, key_len, H, T, scale, drop)
        RL_DISPATCH(relattn_len_bwd_dpos_kernel, bf16, gp, s, (const bf16*)q, (const bf16*)k, (const bf16*)v, posp, u, vb, (const bf16*)dO, lse, (const float*)delta, dposp, key_len, H, T, scale, drop)
    } else {
        RL_DISPATCH(relattn_len_bwd_dq_kernel, float, gq, s, (const float*)q, (const float*)k, (const float*)v, posp, u, vb, (const float*)o, (const float*)dO, lse, delta, (float*)dq, du, dvb, key_len, H, T, scale, drop)
        RL_DISPATCH(relattn_len_bwd_dkv_kernel, float, gq, s, (const float*)q, (const float*)k, (const float*)v, posp, u, vb, (const float*)dO, lse, (const float*)delta, (float*)dk, (float*)dv, key_len, H, T, scale, drop)
        RL_DISPATCH(relattn_len_bwd_dpos_kernel, float, gp, s, (const float*)q, (const float*)k, (const float*)v, posp, u, vb, (const float*)dO, lse, (const float*)delta, dposp, key_len, H, T, scale, drop)
    }
    return launch_rc();
}
