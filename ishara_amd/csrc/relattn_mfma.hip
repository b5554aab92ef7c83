// MFMA forward of the relative-position attention with per-clip key lengths (bf16, head dim 32 / 64, any T >= 1): the kernel the masked route
// of relattn_len.hip's relattn_route runs in place of relattn_len_fwd_kernel.  v_mfma_f32_16x16x32_bf16 throughout, fp32 accumulation.
//
// A workgroup = 4 waves = 64 queries of one (batch, head); a wave owns 16 queries.  Keys are swept in chunks of RM_KC = 32 over
// ceil(n[b] / 32) chunks only (n[b] = clamp(key_len[b], 0, T)); a chunk's K rows, V rows (transposed on the way in) and the window of posp rows
// it needs are staged in LDS, single-buffered, posp converted from the workspace's fp32 to bf16 on the way in.
//   Scores, transposed as in attention_mfma.hip (a lane holds 4 consecutive keys of ONE query, so the online softmax needs two cross-lane
//   shuffles per chunk and the exponentiated tile is the B operand of the second product as it stands):
//     content    S^T = K (Q+u)^T            A = K tile [16 keys x dh] from LDS, B = (Q+u)^T kept in registers (rounded to bf16 once)
//     positional G^T = Pwin (Q+vb)^T        Pwin = the 48 posp rows T-1-(iw+15)+j0 ... of the wave's 16 queries x 32 keys (rows outside [0, 2T-2]
//                                           read as zero), three 16-row tiles; then the SKEW s_pos[key jj][query c] = G^T[15 - c + jj][c]
//                                           through a per-wave fp32 LDS tile (row stride 18 floats: writes and skewed reads at most 2-way)
//   softmax on (content + positional) * scale with the keys >= n[b] at the finite -1e30f sentinel (exp gives exactly 0; every swept chunk
//   starts below n[b], so a row's running maximum is a real score from its first chunk on); dropout by the family's hash (row key
//   (b*H+h)*T+i, column = key, 8-bit threshold: rng_keep_q); P rounded to bf16, O^T += V^T P^T with the k-slot order {4g..4g+3} U {16+4g..16+4g+3}
//   matched on the V^T fragment reads.
// n[b] = 0: no chunk runs, o = 0, lse = ATT_DEAD_LSE.  Nothing at or past key n[b] is read into a sum (staged as zero).
// Rounding points the lane kernels do not have: q+u, q+vb, posp and P to bf16 (tests/relattn_len_parity.py restates them for the bounds).
#include "attention_mfma.h"

#define RM_QB 64      // queries per workgroup
#define RM_KC 32      // keys per chunk
#define RM_WIN 96     // staged posp rows per chunk: RM_QB + RM_KC - 1 = 95 used, the 96th completes the last wave's third tile (never selected)
#define RM_GS 18      // row stride (floats) of the per-wave skew tile

template <int DH>
__global__ __launch_bounds__(256) void relattn_len_fwd_mfma_kernel(const bf16* __restrict__ q, const bf16* __restrict__ k, const bf16* __restrict__ v,
                                                                   const float* __restrict__ posp, const float* __restrict__ u, const float* __restrict__ vb,
                                                                   bf16* __restrict__ o, float* __restrict__ lse, const int* __restrict__ key_len,
                                                                   int H, int Tn, float scale, DropSpec drop) {
    constexpr int KS = DH / 32;      // MFMA k-steps over the head dimension
    constexpr int DT = DH / 16;      // 16-wide output tiles
    constexpr int KLD = DH + 8;      // K / posp row stride (bf16): 80-B / 144-B rows, conflict-free 16-byte fragment reads
    constexpr int VLD = RM_KC + 8;   // V^T row stride (bf16)
    constexpr int PR = DH / 8;       // 16-byte pieces per row
    __shared__ __attribute__((aligned(16))) bf16 Ks[RM_KC * KLD];
    __shared__ __attribute__((aligned(16))) bf16 Vs[DH * VLD];
    __shared__ __attribute__((aligned(16))) bf16 Ps[RM_WIN * KLD];
    __shared__ float Gs[4][48 * RM_GS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, g = lane >> 4, c = lane & 15;
    const int d = H * DH, bh = blockIdx.y, b = bh / H, h = bh - b * H;
    const int i0 = blockIdx.x * RM_QB, iw = i0 + 16 * wid, qi = iw + c;
    const int n = attn_key_count(key_len, b, Tn);
    const bf16* kb = k + (size_t)b * Tn * d + h * DH;
    const bf16* vbase = v + (size_t)b * Tn * d + h * DH;

    // (q + u)^T and (q + vb)^T fragments: B[k = 8g + j][col c] = row min(qi, T-1), columns 32s + 8g + j
    bf16x8 qu[KS], qv[KS];
    {
        const bf16* qp = q + ((size_t)b * Tn + min(qi, Tn - 1)) * d + h * DH;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int e = 32 * s + 8 * g + j;
                const float x = (float)qp[e];
                qu[s][j] = (bf16)(x + u[h * DH + e]);
                qv[s][j] = (bf16)(x + vb[h * DH + e]);
            }
    }
    f32x4 acc_o[DT];
#pragma unroll
    for (int t = 0; t < DT; ++t) acc_o[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;
    const uint32_t rk = rng_row_key(drop.key, (uint32_t)(bh * Tn + qi));
    float* Gw = Gs[wid];

    for (int j0 = 0; j0 < n; j0 += RM_KC) {
        const int rbase = Tn - 1 - (i0 + RM_QB - 1) + j0;      // posp row of Ps[0]
        __syncthreads();
        for (int pi = tid; pi < RM_KC * PR; pi += 256) {       // K rows as stored; V transposed: Vs[dv][key]
            const int key = pi / PR, part = pi - key * PR, j = j0 + key;
            u32x4 kr = u32x4{0u, 0u, 0u, 0u};
            bf16x8 vr;
#pragma unroll
            for (int e = 0; e < 8; ++e) vr[e] = (bf16)0.f;
            if (j < n) {
                kr = *reinterpret_cast<const u32x4*>(kb + (size_t)j * d + part * 8);
                vr = *reinterpret_cast<const bf16x8*>(vbase + (size_t)j * d + part * 8);
            }
            *reinterpret_cast<u32x4*>(&Ks[key * KLD + part * 8]) = kr;
#pragma unroll
            for (int e = 0; e < 8; ++e) Vs[(part * 8 + e) * VLD + key] = vr[e];
        }
        for (int pi = tid; pi < RM_WIN * PR; pi += 256) {      // the posp window, fp32 -> bf16
            const int rr = pi / PR, part = pi - rr * PR, r = rbase + rr;
            u32x4 w = u32x4{0u, 0u, 0u, 0u};
            if (r >= 0 && r < 2 * Tn - 1) {
                const float* src = posp + (size_t)r * d + h * DH + part * 8;
                const f32x4 a = *reinterpret_cast<const f32x4*>(src), bq = *reinterpret_cast<const f32x4*>(src + 4);
                w = u32x4{pk2(a[0], a[1]), pk2(a[2], a[3]), pk2(bq[0], bq[1]), pk2(bq[2], bq[3])};
            }
            *reinterpret_cast<u32x4*>(&Ps[rr * KLD + part * 8]) = w;
        }
        __syncthreads();
        // ---- G^T = Pwin (Q+vb)^T: the wave's 48 window rows start at Ps row 48 - 16 * wid
        const int pw = 48 - 16 * wid;
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            f32x4 ga = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const bf16x8 pf = *reinterpret_cast<const bf16x8*>(&Ps[(pw + 16 * t + c) * KLD + 32 * s + 8 * g]);
                ga = af_mfma(pf, qv[s], ga);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Gw[(16 * t + 4 * g + r) * RM_GS + c] = ga[r];      // C[row = window row 16t + 4g + r][col = query c]
        }
        // ---- S^T = K (Q+u)^T
        f32x4 sacc[2];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            sacc[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8*>(&Ks[(16 * kt + c) * KLD + 32 * s + 8 * g]);
                sacc[kt] = af_mfma(kf, qu[s], sacc[kt]);
            }
        }
        __syncthreads();      // the skew tile is read by other lanes than wrote it
        // ---- scores of (query c, keys j0 + 16kt + 4g + r), the skewed positional part added
        float mx = -1e30f;
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int jj = 16 * kt + 4 * g + r;
                float s = (sacc[kt][r] + Gw[(15 - c + jj) * RM_GS + c]) * scale;
                if (j0 + jj >= n) s = -1e30f;
                sacc[kt][r] = s;
                mx = fmaxf(mx, s);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mn = fmaxf(m_run, mx);
        const float corr = __expf(m_run - mn);
        m_run = mn;
        l_run *= corr;
#pragma unroll
        for (int t = 0; t < DT; ++t) acc_o[t] *= corr;
        float p[2][4];
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = j0 + 16 * kt + 4 * g + r;
                const float pv = j < n ? __expf(sacc[kt][r] - mn) : 0.f;
                l_run += pv;
                p[kt][r] = (drop.thr == 0u || rng_keep_q(rk, (uint32_t)j, drop.thr)) ? pv : 0.f;
            }
        const u32x4 w = u32x4{pk2(p[0][0], p[0][1]), pk2(p[0][2], p[0][3]), pk2(p[1][0], p[1][1]), pk2(p[1][2], p[1][3])};
        const bf16x8 pb = __builtin_bit_cast(bf16x8, w);
        // ---- O^T += V^T P^T
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            const bf16* vrow = &Vs[(16 * t + c) * VLD + 4 * g];
            const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow);
            const u32x2 hi = *reinterpret_cast<const u32x2*>(vrow + 16);
            const bf16x8 vf = __builtin_bit_cast(bf16x8, (u32x4){lo.x, lo.y, hi.x, hi.y});
            acc_o[t] = af_mfma(vf, pb, acc_o[t]);
        }
    }
    // ---- normalise and store: lane = (query c, columns 16t + 4g + r)
    float l = l_run;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (qi < Tn) {
        const bool dead = !(l > 0.f);
        const float inv = dead ? 0.f : drop.scale / l;
        bf16* orow = o + ((size_t)b * Tn + qi) * d + h * DH;
#pragma unroll
        for (int t = 0; t < DT; ++t) {
            bf16x4 w4;
#pragma unroll
            for (int r = 0; r < 4; ++r) w4[r] = (bf16)(acc_o[t][r] * inv);
            *reinterpret_cast<bf16x4*>(orow + 16 * t + 4 * g) = w4;
        }
        if (g == 0) lse[(size_t)bh * Tn + qi] = dead ? ATT_DEAD_LSE : m_run + __logf(l);
    }
}

// bf16, dh 32 or 64 (the route's), rows 16-byte aligned (d % 8 == 0)
int launch_relattn_len_fwd_mfma(const void* q, const void* k, const void* v, const float* posp, const float* u, const float* vb, void* o, float* lse,
                                const int* key_len, int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s) {
    const dim3 grid((T + RM_QB - 1) / RM_QB, B * H);
    if (dh == 32) hipLaunchKernelGGL((relattn_len_fwd_mfma_kernel<32>), grid, dim3(256), 0, s, (const bf16*)q, (const bf16*)k, (const bf16*)v, posp, u, vb, (bf16*)o, lse, key_len, H, T, scale, drop);
    else hipLaunchKernelGGL((relattn_len_fwd_mfma_kernel<64>), grid, dim3(256), 0, s, (const bf16*)q, (const bf16*)k, (const bf16*)v, posp, u, vb, (bf16*)o, lse, key_len, H, T, scale, drop);
    return launch_rc();
}
