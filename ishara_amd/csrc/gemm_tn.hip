// gemm_tn : dW[K,N] += opA(A)[M,K]^T . opB(B)[M,N]         wgrad (+ bias grad), split over M (gfx950 / CDNA4).
// The register-transposing kernel, the bf16 transposed-read kernel with its per-sample-affine variant, the split plans, the
// kernel route, launcher, flush and profiler key.  Tile structure and operand staging: gemm_nt.hip, gemm_tile.h.
#include "gemm_tile.h"

// ---------------------------------------------------------------------------------
// TN kernel (wgrad).  grid = (tiles_k * tiles_n, splits).  Both operands are staged
// TRANSPOSED into LDS ([feature row][m contiguous]) so the MFMA fragment reads are the
// same as in the NT kernel; swizzle SW=1 keeps both the 8-byte transposed writes and
// the 16-byte fragment reads at <= 2-way bank conflicts.
// ---------------------------------------------------------------------------------
template <typename T, typename TM>
DEVI void stage_t_load(const T* __restrict__ base, int ld, int m_end, int cols, int mbase, int col0, bool vec_ok,
                       int op, const OpArgs& oa, int tid, u32x4 (&out)[4], float* colsum) {
    // bf16 TM: thread -> kc = tid&15 (8 cols), mg = tid>>4 (4 rows of 64) ; out[e] holds rows for cols 2e,2e+1 (uint2 each)
    // f32  TM: thread -> kc = tid&31 (4 cols), mg = tid>>5 (4 rows of 32) ; out[e] = 4 rows of col e
    constexpr int EPC = MmaCfg<TM>::EPC;
    const int kc = is_bf16_t<TM>::value ? (tid & 15) : (tid & 31);
    const int mg = is_bf16_t<TM>::value ? (tid >> 4) : (tid >> 5);
    float v[4][EPC];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = mbase + 4 * mg + r, col = col0 + kc * EPC;
        load_row_chunk<T, EPC>(base, ld, m_end, cols, m, col, vec_ok, v[r]);
        if (op != OP_NONE) {
            apply_op<EPC>(op, v[r], m, col, oa);
            if (m >= m_end) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) v[r][e] = 0.f;
            } else if (col + EPC > cols) {
#pragma unroll
                for (int e = 0; e < EPC; ++e) if (col + e >= cols) v[r][e] = 0.f;
            }
        }
    }
    if (colsum) {
#pragma unroll
        for (int e = 0; e < EPC; ++e) colsum[e] += (v[0][e] + v[1][e]) + (v[2][e] + v[3][e]);
    }
    if constexpr (is_bf16_t<TM>::value) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            out[e].x = pack_bf16x2(v[0][2 * e], v[1][2 * e]);         out[e].y = pack_bf16x2(v[2][2 * e], v[3][2 * e]);
            out[e].z = pack_bf16x2(v[0][2 * e + 1], v[1][2 * e + 1]); out[e].w = pack_bf16x2(v[2][2 * e + 1], v[3][2 * e + 1]);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            out[e].x = __float_as_uint(v[0][e]); out[e].y = __float_as_uint(v[1][e]);
            out[e].z = __float_as_uint(v[2][e]); out[e].w = __float_as_uint(v[3][e]);
        }
    }
}

template <typename TM>
DEVI void stage_t_store(char* lds, int tid, const u32x4 (&r)[4]) {
    if constexpr (is_bf16_t<TM>::value) {
        const int kc = tid & 15, mg = tid >> 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int row = 8 * kc + 2 * e + h;
                const int off = row * 128 + (((mg >> 1) ^ swz<1>(row)) << 4) + ((mg & 1) << 3);
                *reinterpret_cast<u32x2*>(lds + off) = h == 0 ? u32x2{r[e].x, r[e].y} : u32x2{r[e].z, r[e].w};
            }
        }
    } else {
        const int kc = tid & 31, mg = tid >> 5;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = 4 * kc + e;
            *reinterpret_cast<u32x4*>(lds + row * 128 + ((mg ^ swz<1>(row)) << 4)) = r[e];
        }
    }
}

template <typename TA, typename TB, typename TM>
__global__ __launch_bounds__(256) void gemm_tn_kernel(const TA* __restrict__ A, const TB* __restrict__ B,
                                                      float* __restrict__ slab, float* __restrict__ bias_slab,
                                                      int M, int Ka, int Nb, int rows_per_split, int a_vec_ok, int b_vec_ok,
                                                      int opA, int opB, OpArgs oa, OpArgs ob, int dbg) {
    __shared__ __attribute__((aligned(16))) char smem[65536];
    constexpr int EPC = MmaCfg<TM>::EPC, MC = MmaCfg<TM>::BK;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
    const int nNt = (Nb + 127) >> 7;
    const int kt = blockIdx.x / nNt, nt = blockIdx.x % nNt;
    const int k0 = kt << 7, n0 = nt << 7;
    const int split = blockIdx.y;
    const int m_beg = split * rows_per_split;
    const int m_end = min(M, m_beg + rows_per_split);
    const int nmc = (m_end - m_beg + MC - 1) / MC;
    const bool want_bias = (bias_slab != nullptr) && (kt == 0);

    u32x4 ra[4], rb[4];
    float csum[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) csum[e] = 0.f;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (nmc > 0) {
        stage_t_load<TA, TM>(A, Ka, m_end, Ka, m_beg, k0, a_vec_ok != 0, opA, oa, tid, ra, nullptr);
        stage_t_load<TB, TM>(B, Nb, m_end, Nb, m_beg, n0, b_vec_ok != 0, opB, ob, tid, rb, want_bias ? csum : nullptr);
        stage_t_store<TM>(smem, tid, ra);
        stage_t_store<TM>(smem + 16384, tid, rb);
    }
    __syncthreads();
    for (int mc = 0; mc < nmc; ++mc) {
        const bool more = mc + 1 < nmc;
        if (more && !(dbg & 4)) {
            stage_t_load<TA, TM>(A, Ka, m_end, Ka, m_beg + (mc + 1) * MC, k0, a_vec_ok != 0, opA, oa, tid, ra, nullptr);
            stage_t_load<TB, TM>(B, Nb, m_end, Nb, m_beg + (mc + 1) * MC, n0, b_vec_ok != 0, opB, ob, tid, rb, want_bias ? csum : nullptr);
        }
        const char* sa = smem + (mc & 1) * 32768;
        if (!(dbg & 1)) mma_tile<TM, 1>(sa, sa + 16384, wr, wc, lane, acc);
        if (more && !(dbg & 2)) {
            char* sn = smem + ((mc + 1) & 1) * 32768;
            stage_t_store<TM>(sn, tid, ra);
            stage_t_store<TM>(sn + 16384, tid, rb);
        }
        __syncthreads();
    }

    float* out = slab + (size_t)split * Ka * Nb;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kk = k0 + wr * 64 + 16 * i + 4 * (lane >> 4) + r;
                const int nn = n0 + wc * 64 + 16 * j + (lane & 15);
                if (kk < Ka && nn < Nb) out[(size_t)kk * Nb + nn] = acc[i][j][r];
            }

    if (want_bias) {   // block-reduce the per-thread column sums (uniform branch: kt is per-block)
        float* red = reinterpret_cast<float*>(smem);       // [groups][128]
        constexpr int GROUPS = is_bf16_t<TM>::value ? 16 : 8;
        const int kc = is_bf16_t<TM>::value ? (tid & 15) : (tid & 31);
        const int mg = is_bf16_t<TM>::value ? (tid >> 4) : (tid >> 5);
#pragma unroll
        for (int e = 0; e < EPC; ++e) red[mg * 128 + kc * EPC + e] = csum[e];
        __syncthreads();
        if (tid < 128) {
            float sacc = 0.f;
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) sacc += red[g * 128 + tid];
            if (n0 + tid < Nb) bias_slab[(size_t)split * Nb + n0 + tid] = sacc;
        }
    }
}

// ---------------------------------------------------------------------------------
// TN kernel, bf16, LDS-DMA + hardware-transposed fragment reads (the common wgrad case: no
// operand transform, M % 64 == 0, Ka % 128 == 0, Nb % 128 == 0).
// Both operands are [m][feature] row-major in HBM and the MFMA reduction index is m, i.e. the
// fragments are COLUMNS of the stored tiles.  Instead of transposing through registers, the
// 32-row x 128-column tiles (256-byte rows) are copied as they are by global_load_lds_dwordx4
// into a 4-deep LDS ring (three tiles in flight, two workgroups per CU), and each fragment is fetched with two
// ds_read_b64_tr_b16 (a 4-row x 16-column block delivered column-major).  The 32-byte column
// blocks of a row are XOR-swizzled with f(row) = (row&3) | ((row>>3)&1)<<2 — applied on the
// SOURCE address of the DMA and on the read — so the 8 rows a 32-lane half reads land in 8
// different 32-byte bank groups (conflict-free).  The bias gradient (column sums of dY) is
// accumulated from the B fragments already in registers.  M is split over workgroups; each writes
// its 128x128 fp32 partial to a slab with coalesced 16-byte stores (an all-at-once fp32-atomic
// epilogue measured 40 us for 32 MB, the chip-wide atomic rate) and reduce_slabs_kernel sums them.
// ---------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;
#define TR_STAGE 16384          // A 32 rows x 256 B + B 32 rows x 256 B
#define TR_ROWS 32
#define TR_AUX 0             // cache policy of the operand DMA: 0 = default: the tiles of one M-split share the operand rows through L2 (non-temporal, 2, measured 2.38 -> 2.87 ms/step of wgrad)
#define TR_NSTAGE 4          // measured: 3 stages (3 workgroups/CU) 116 us, 4 stages (2/CU) 90 us, 5 stages (80 KB, 1-2/CU) 94 us per wgrad

DEVI int tr_f(int row) { return (row & 3) | (((row >> 3) & 1) << 2); }

DEVI void tr_issue(const bf16* __restrict__ A, const bf16* __restrict__ B, int Ka, int Nb, int k0, int n0, int mrow0,
                   char* stage, int wid, int lane) {
    const int r = lane >> 4, sp = lane & 15;            // row within a 4-row piece, physical 16-byte slot
#pragma unroll
    for (int u = 0; u < 2; ++u) {                        // 8 four-row pieces per operand; wave takes wid, wid+4
        const int pc = wid + 4 * u;
        const int row = 4 * pc + r;
        const int col = (((sp >> 1) ^ tr_f(row)) << 4) + ((sp & 1) << 3);     // logical column of physical slot sp
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(A + (size_t)(mrow0 + row) * Ka + k0 + col),
                                         (__attribute__((address_space(3))) void*)(stage + pc * 1024), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(B + (size_t)(mrow0 + row) * Nb + n0 + col),
                                         (__attribute__((address_space(3))) void*)(stage + 8192 + pc * 1024), 16, 0, 0);
    }
}

// fragment of column block lb (16 columns), k-step s (32 rows): lane (g,q,p) addresses row 32s+8g+4h+q, 8 bytes at p
DEVI bf16x8 tr_frag(const char* tile, int lb, int s, int lane) {
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const int r0 = 32 * s + 8 * g + q, r1 = r0 + 4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + r0 * 256 + ((lb ^ tr_f(r0)) << 5) + (pp << 3)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(tile + r1 * 256 + ((lb ^ tr_f(r1)) << 5) + (pp << 3)));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

typedef __attribute__((ext_vector_type(2))) unsigned tn_u32x2;
struct TrFrags { u32x4 a[4], b[4]; };
// fragment reads of the A (offset 0) and B (offset 8192) tiles of ring slot SLOT, as inline asm (see the kernel comment)
template <int SLOT>
DEVI void tr_read_asm(const unsigned (&fa)[4], const unsigned (&fb)[4], TrFrags& f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        tn_u32x2 lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(fa[i]), "n"(SLOT * TR_STAGE));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(fa[i]), "n"(SLOT * TR_STAGE + 1024));
        f.a[i] = u32x4{lo.x, lo.y, hi.x, hi.y};
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        tn_u32x2 lo, hi;
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(fb[j]), "n"(SLOT * TR_STAGE + 8192));
        asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(fb[j]), "n"(SLOT * TR_STAGE + 8192 + 1024));
        f.b[j] = u32x4{lo.x, lo.y, hi.x, hi.y};
    }
}
// the reads above have landed: the fragments pass through the wait so that their consumers are ordered behind it
DEVI void tr_wait(TrFrags& f) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(f.a[0]), "+v"(f.a[1]), "+v"(f.a[2]), "+v"(f.a[3]), "+v"(f.b[0]), "+v"(f.b[1]), "+v"(f.b[2]), "+v"(f.b[3]));
}

// The slab sums of the PREVIOUS weight-gradient GEMM ride along as extra workgroups of the next one (blockIdx.x >= nmain): the sums are
// ~5 us kernels that leave the chip idle, 59 of them per step; here they run beside the GEMM's workgroups (two slab buffers alternate).
struct TnRed { const float* slab; float* out0; float* out1; int n0, n, splits; size_t stride; int nb, nbv, nmain; int inl; };   // inl: no rider workgroups — every main workgroup sums its share after its tile (PSA: one workgroup per CU, riders could not run beside them)
DEVI void tn_reduce_block(const TnRed& r, int rb, int nrb, float4 (*red)[32]) {
    constexpr int SL = 8, CQ = 32;                       // the layout of reduce_slabs_cols_kernel<8, 32>
    const int tid = threadIdx.x, cq = tid % CQ, sl = tid / CQ;
    for (int grp = rb; grp * (CQ * 4) < r.n; grp += nrb) {
        const int col = grp * (CQ * 4) + cq * 4;
        const int cin = r.nb ? (col < r.n0 ? col % r.nb : col - r.n0) : 0;
        const bool valid = col < r.n && (r.nb == 0 || cin < r.nbv);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (valid) {
            for (int s0 = sl; s0 < r.splits; s0 += SL * 8) {
                float4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int sidx = s0 + SL * u;
                    v[u] = sidx < r.splits ? *reinterpret_cast<const float4*>(r.slab + (size_t)sidx * r.stride + col) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w; }
            }
        }
        red[sl][cq] = acc;
        __syncthreads();
        if (sl == 0 && valid) {
            float4 t = red[0][cq];
#pragma unroll
            for (int w = 1; w < SL; ++w) { t.x += red[w][cq].x; t.y += red[w][cq].y; t.z += red[w][cq].z; t.w += red[w][cq].w; }
            float* dst = col < r.n0 ? (r.nb ? r.out0 + (size_t)(col / r.nb) * r.nbv + cin : r.out0 + col) : r.out1 + (col - r.n0);
            dst[0] += t.x; dst[1] += t.y; dst[2] += t.z; dst[3] += t.w;
        }
        __syncthreads();
    }
}

template <int CTRL> DEVI float tn_dpp_add(float v) {
    return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// One sample of the split is complete (PSA).  Its accumulator is folded into the running total with the sample's affine, and the
// statistics of the gradient of the transformed operand are emitted — but not on the spot: a pause of the whole workgroup (~700 VALU
// instructions per wave) lets the 3-stage operand ring run dry, and refilling it cost more than the arithmetic (first version: 4 us per
// boundary, 77 us per launch against 41 without).  tn_psa_begin parks the finished accumulator (hold) and the sample's column sums; the
// four 16-row chunks are processed by tn_psa_chunk<I> in the next four steps, in the same basic block as their MFMAs (samples are a
// multiple of four stages long, so chunk I always sits in step copy I of the 4x unrolled loop).  Two accumulator sets alternating between
// samples (no parking) made hipcc spill 250 registers per lane to scratch.  The statistics go to LDS (po: this lane's R quad of the
// sample's 384-float record [4 waves x 64 R | 128 G], asm stores: a builtin LDS access would wait for all operand DMA) and to memory
// after the loop — global stores in the loop would sit in vmcnt between the DMAs and be waited for by the steps' vmcnt(8).
DEVI void tn_psa_begin(f32x4 (&acc)[4][4], f32x4 (&hold)[4][4], f32x4 (&gacc)[4], float (&ctot)[4], float (&gbh)[4], unsigned gaddr,
                       bool psa_g, const float* __restrict__ brs, int sample, int lane, u32x4 z8) {
    // column sums of B over the sample's rows: an MFMA with an all-ones A operand per B fragment (every accumulator row holds them — no
    // cross-lane fold; summing the unpacked fragments on the VALU in every wave cost 10 us per launch)
#pragma unroll
    for (int j = 0; j < 4; ++j) { gbh[j] = gacc[j][0]; gacc[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (psa_g) {
        const float sc = brs ? brs[sample] : 1.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) ctot[j] += sc * gbh[j];
        if ((lane >> 4) == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("ds_write_b32 %0, %1" :: "v"(gaddr + 64u * j), "v"(gbh[j]) : "memory");
        }
    }
    // park the finished accumulator and clear it ON THE MATRIX PIPE (z8 = an all-zero operand the compiler cannot see through):
    // hold = 0 x 0 + acc, acc = 0 x 0 + 0 — 32 MFMAs the pipe has room for, instead of ~200 accumulator-register moves on the VALU
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            hold[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, z8), __builtin_bit_cast(bf16x8, z8), acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, z8), __builtin_bit_cast(bf16x8, z8), f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        }
}
// The running total lives in LDS (tot_lds: this lane's 16-byte slot of the wave's [16 tiles][64 lanes] f32x4 block): with it in registers
// the kernel needed 530 of the 512 registers a wave can have.
template <int I>
DEVI void tn_psa_chunk(const f32x4 (&hold)[4][4], unsigned tot_lds, const tn_u32x2 (&wv)[4][4], const float (&gbh)[4], unsigned prow, unsigned orow, int lane) {
    f32x4 p4, q4, tot[1][4];
    asm volatile("ds_read_b128 %0, %1" : "=v"(p4) : "v"(prow + 64u * I));
    asm volatile("ds_read_b128 %0, %1 offset:512" : "=v"(q4) : "v"(prow + 64u * I));
    const unsigned ta = tot_lds + 4096u * I;
    asm volatile("ds_read_b128 %0, %1" : "=v"(tot[0][0]) : "v"(ta));
    asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(tot[0][1]) : "v"(ta));
    asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(tot[0][2]) : "v"(ta));
    asm volatile("ds_read_b128 %0, %1 offset:3072" : "=v"(tot[0][3]) : "v"(ta));
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(p4), "+v"(q4), "+v"(tot[0][0]), "+v"(tot[0][1]), "+v"(tot[0][2]), "+v"(tot[0][3]));
    f32x4 rr = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float w0 = __uint_as_float(wv[I][j].x << 16), w1 = __uint_as_float(wv[I][j].x & 0xffff0000u);
        const float w2 = __uint_as_float(wv[I][j].y << 16), w3 = __uint_as_float(wv[I][j].y & 0xffff0000u);
        const f32x4 a = hold[I][j];
        const f32x4 w4 = {w0, w1, w2, w3};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            tot[0][j][r] += p4[r] * a[r] + q4[r] * gbh[j];
            rr[r] += w4[r] * a[r];
        }
    }
    asm volatile("ds_write_b128 %0, %1" :: "v"(ta), "v"(tot[0][0]) : "memory");
    asm volatile("ds_write_b128 %0, %1 offset:1024" :: "v"(ta), "v"(tot[0][1]) : "memory");
    asm volatile("ds_write_b128 %0, %1 offset:2048" :: "v"(ta), "v"(tot[0][2]) : "memory");
    asm volatile("ds_write_b128 %0, %1 offset:3072" :: "v"(ta), "v"(tot[0][3]) : "memory");
#pragma unroll
    for (int r = 0; r < 4; ++r) {                         // sum over the 16 column lanes of the row (quad swaps, half mirror, mirror)
        float v = rr[r];
        v = tn_dpp_add<0xB1>(v); v = tn_dpp_add<0x4E>(v); v = tn_dpp_add<0x141>(v); v = tn_dpp_add<0x140>(v);
        rr[r] = v;
    }
    if ((lane & 15) == 0) asm volatile("ds_write_b128 %0, %1" :: "v"(orow + 64u * I), "v"(rr) : "memory");
}

#define TN_PSA_MAXS 8          // samples per M-split the per-sample-affine variant stages coefficients for
// DBG = 1: the ablation bits of tools/gemm_ablate.py are honoured (kept out of the production loop); BRS: weighted bias sum;
// PSA: per-sample affine of the A operand + the BatchNorm / ECA backward statistics (TnPsa, kernels.h): one workgroup per CU (the per-sample
// accumulator, the running total and the weight tile take 192 registers)
template <int DBG, bool BRS = false, bool PSA = false>
__global__ __launch_bounds__(256, PSA ? 1 : 2) void gemm_tn_tr_kernel(const bf16* __restrict__ A, const bf16* __restrict__ B,
                                                         float* __restrict__ out, float* __restrict__ dbias,
                                                         int M, int Ka, int Nb, int rows_per_split, int tiles, int nsplits, int dbg,
                                                         const float* __restrict__ brs, int brsT, TnRed prev, TnPsa psa) {
    // brs != nullptr: the bias gradient is the column sum of brs[m / brsT] * B[m,:] (drop-path scale of the sample a row belongs to;
    // brsT % 32 == 0, so the 32 rows of a stage share it)
    // slab layout: [split][Ka*Nb weight partial | Nb bias partial] so that ONE reduction launch sums both
    const size_t sstride = (size_t)Ka * Nb + Nb;
    __shared__ __attribute__((aligned(16))) char smem[TR_NSTAGE * TR_STAGE];
    __shared__ __attribute__((aligned(16))) float pq_tab[PSA ? TN_PSA_MAXS * 256 : 4];     // [sample of this split][P of the tile's 128 rows | Q]
    __shared__ __attribute__((aligned(16))) float psa_out[PSA ? TN_PSA_MAXS * 384 : 4];    // [sample of this split][R: 4 waves x 64 rows | G: 128 columns]
    __shared__ __attribute__((aligned(16))) f32x4 tot_tab[PSA ? 4 * 16 * 64 : 1];          // [wave][tile i*4+j][lane]: the running total (sum over finished samples)
    if (prev.nmain > 0 && !prev.inl && (int)blockIdx.x >= prev.nmain) {        // a rider: sums a slice of the previous launch's slabs
        tn_reduce_block(prev, (int)blockIdx.x - prev.nmain, (int)gridDim.x - prev.nmain, reinterpret_cast<float4 (*)[32]>(smem));
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    const int nNt = Nb >> 7;
    // XCD-aware mapping (blocks b, b+8 share an XCD / L2): the `tiles` output tiles of one M-split read the same
    // A and dY rows, so they are dealt to ONE XCD back to back; consecutive splits go to different XCDs.
    int tile, split;
    {
        const int id = blockIdx.x, xcd = id & 7, j = id >> 3;
        if ((nsplits & 7) == 0) { split = (j / tiles) * 8 + xcd; tile = j % tiles; }
        else { split = id / tiles; tile = id % tiles; }
    }
    const int kt = tile / nNt, nt = tile % nNt;
    const int k0 = kt << 7, n0 = nt << 7;
    const int m_beg = split * rows_per_split;
    const int m_end = min(M, m_beg + rows_per_split);
    const int nmc = max(0, m_end - m_beg) / TR_ROWS;      // whole 32-row tiles (launcher guarantees)
    const bool want_bias = (dbias != nullptr) && (kt == 0) && (wr == 0);

    f32x4 acc[4][4], hold[4][4];           // hold (PSA): the previous sample's accumulator while its chunks are processed
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) { acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; hold[i][j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    float csum[4] = {0.f, 0.f, 0.f, 0.f};
    // weighted bias sum: csum collects the rows of the current sample; at a sample boundary (every brsT / 32 stages) it is folded into
    // ctot with that sample's scale — one scalar load per sample instead of one per stage (a scalar load in the step loop shares
    // lgkmcnt with the fragment reads and stalls them)
    float ctot[4] = {0.f, 0.f, 0.f, 0.f};
    const int seg_stages = PSA ? psa.T / TR_ROWS : (BRS ? brsT / TR_ROWS : 0);
    const int seg_iters = seg_stages / 4;                    // PSA: samples are a multiple of 4 stages (launcher)
    int seg_left = PSA ? seg_iters : (BRS ? seg_stages - (m_beg % brsT) / TR_ROWS : -1);      // PSA: splits are whole samples (launcher)
    int seg_sample = PSA ? m_beg / psa.T : (BRS ? m_beg / brsT : 0);
    // ---- PSA state: tot = sum over finished samples of P[b] * acc_b + Q[b] x colsum_b ; wv = this wave's 64x64 block of W in the
    // accumulator layout (row 16i + 4(lane>>4) + r, column 16j + (lane&15))
    tn_u32x2 wv[4][4];                                       // bf16 pairs (rows r0|r1, r2|r3)
    float gbh[4] = {0.f, 0.f, 0.f, 0.f};
    f32x4 gacc[4];                                           // column sums of the current sample's B rows (ones x B fragments)
#pragma unroll
    for (int j = 0; j < 4; ++j) gacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const u32x4 ones8 = {0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u};
    bool first = false;                                      // the running iteration is the first of a sample whose predecessor is parked
    u32x4 z8 = {0u, 0u, 0u, 0u};                             // an all-zero MFMA operand, opaque to the compiler (tn_psa_begin)
    asm volatile("" : "+v"(z8));
    unsigned pq_hold = 0, po_hold = 0;
    unsigned pq_row = (unsigned)(uintptr_t)pq_tab + 4u * (wr * 64 + 4 * (lane >> 4));     // LDS byte address of this lane's coefficient quad
    unsigned po_row = (unsigned)(uintptr_t)psa_out + 4u * (wid * 64 + 4 * (lane >> 4));    // ... of its R quad, and of its G column
    unsigned po_g = (unsigned)(uintptr_t)psa_out + 4u * (256 + wc * 64 + (lane & 15));
    const unsigned tot_lds = (unsigned)(uintptr_t)tot_tab + 16u * (wid * 16 * 64 + lane);
    const bool psa_g = PSA && kt == 0 && wr == 0;            // the waves that publish G[b, :] and own the bias sum
    float tv[PSA ? TN_PSA_MAXS : 1];
    if constexpr (PSA) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) tot_tab[(wid * 16 + i * 4 + j) * 64 + lane] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int ns = nmc / seg_stages;
        const float* src = (tid < 128 ? psa.P : psa.Q) + (size_t)seg_sample * Ka + k0 + (tid & 127);
#pragma unroll
        for (int sidx = 0; sidx < TN_PSA_MAXS; ++sidx) tv[sidx] = (sidx < ns && !(psa.dbg & 4)) ? src[(size_t)sidx * Ka] : 0.f;
        const bf16* wsrc = reinterpret_cast<const bf16*>(psa.W) + (size_t)(k0 + wr * 64 + 4 * (lane >> 4)) * psa.ldw + n0 + wc * 64 + (lane & 15);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned short* wp = reinterpret_cast<const unsigned short*>(wsrc) + (size_t)(16 * i) * psa.ldw + 16 * j;
                if (psa.dbg & 4) { wv[i][j].x = 0u; wv[i][j].y = 0u; continue; }
                wv[i][j].x = (unsigned)wp[0] | ((unsigned)wp[psa.ldw] << 16);
                wv[i][j].y = (unsigned)wp[2 * (size_t)psa.ldw] | ((unsigned)wp[3 * (size_t)psa.ldw] << 16);
            }
    }
    (void)psa_out; (void)tv;

    // Software pipeline over the 32-row stages (ring of 4 x 16 KB, slots addressed statically: the loop is unrolled by 4):
    // at step mc the MFMAs of stage mc run from fragments already in registers while the transposing LDS reads of stage
    // mc+1 are in flight into the OTHER fragment set (ping-pong, no copies), and stages mc+2 .. mc+4 are in flight from
    // L2/HBM (the slot of stage mc is free as soon as every wave has passed this step's barrier, because its fragments
    // were read and waited for during step mc-1).
    // The fragment reads are inline asm: for the ds_read_tr builtin hipcc puts `s_waitcnt vmcnt(0)` in front of the reads
    // (it cannot tell them from the LDS-DMA writes in flight) and `lgkmcnt(0)` in front of the MFMAs, which serialises
    // the DMA of three stages, the LDS reads and the MFMAs of every step.
    // DMA source pointers of this lane for the NEXT stage to issue (advanced by 32 rows per issue: no 64-bit address
    // arithmetic in the loop); stages are always issued in order 0, 1, 2, ...
    const bf16* pa[2];
    const bf16* pb[2];
    {
        const int r = lane >> 4, sp = lane & 15;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int pc = wid + 4 * u, row = 4 * pc + r;
            const int col = (((sp >> 1) ^ tr_f(row)) << 4) + ((sp & 1) << 3);
            pa[u] = A + (size_t)(m_beg + row) * Ka + k0 + col;
            pb[u] = B + (size_t)(m_beg + row) * Nb + n0 + col;
        }
    }
    const size_t stepA = (size_t)TR_ROWS * Ka, stepB = (size_t)TR_ROWS * Nb;
    // LDS byte addresses of this lane's fragment reads in slot 0 (lane (g,q,p) addresses row 8g+q, +4 rows at +1024)
    unsigned fa[4], fb[4];
    {
        const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3, r0 = 8 * g + q;
        const unsigned base = (unsigned)(uintptr_t)smem + r0 * 256 + (pp << 3);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fa[i] = base + (((wr * 4 + i) ^ tr_f(r0)) << 5);
            fb[i] = base + (((wc * 4 + i) ^ tr_f(r0)) << 5);
        }
    }
    const bool no_dma = DBG != 0 && (dbg & 4) != 0, no_frag = DBG != 0 && (dbg & 2) != 0, no_mma = DBG != 0 && (dbg & 1) != 0;
    const int nmc_run = (DBG != 0 && (dbg & 16) != 0) ? 0 : nmc;
    TrFrags P, Q;
#pragma unroll
    for (int i = 0; i < 4; ++i) { P.a[i] = P.b[i] = Q.a[i] = Q.b[i] = u32x4{0u, 0u, 0u, 0u}; }

#define TN_ISSUE(SLOT, ST)                                                                                               \
    if ((ST) < nmc && !no_dma) {                                                                                         \
        _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                                  \
            const int pc = wid + 4 * u;                                                                                  \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pa[u],                       \
                                             (__attribute__((address_space(3))) void*)(smem + (SLOT) * TR_STAGE + pc * 1024), 16, 0, TR_AUX);        \
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)pb[u],                       \
                                             (__attribute__((address_space(3))) void*)(smem + (SLOT) * TR_STAGE + 8192 + pc * 1024), 16, 0, TR_AUX); \
            pa[u] += stepA; pb[u] += stepB;                                                                              \
        }                                                                                                                \
    }
#define TN_COMPUTE(CUR)                                                                                                  \
    if (PSA) {                                                                                                           \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                    \
            gacc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ones8), __builtin_bit_cast(bf16x8, CUR.b[j]), gacc[j], 0, 0, 0); \
    }                                                                                                                    \
    if (!PSA && want_bias) {                                                                                             \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                                                  \
            float t = 0.f;                                                                                               \
            _Pragma("unroll") for (int e = 0; e < 4; ++e)                                                                \
                t += __uint_as_float(CUR.b[j][e] << 16) + __uint_as_float(CUR.b[j][e] & 0xffff0000u);                    \
            csum[j] += t;                                                                                                \
        }                                                                                                                \
    }                                                                                                                    \
    if (!no_mma) {                                                                                                       \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                                    \
            _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, CUR.a[i]), __builtin_bit_cast(bf16x8, CUR.b[j]), acc[i][j], 0, 0, 0); \
    } else {                                                                                                             \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) acc[i][0][0] += __uint_as_float(CUR.a[i][0]) + __uint_as_float(CUR.b[i][0]); \
    }
    // one step: FULL = at least two younger stages are in flight behind stage mc+U+1 (steady state: no branches)
#define TN_STEP(U, CUR, NXT, FULL, CH)                                                                                   \
    if (FULL || mc + (U) < nmc_run) {                                                                                    \
        if (FULL) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                                                       \
        else {                                                                                                           \
            const int younger = min(nmc - 1, mc + (U) + 3) - (mc + (U) + 1);                                             \
            if (younger >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");                                           \
            else if (younger == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                                      \
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                        \
        }                                                                                                                \
        __builtin_amdgcn_s_barrier();                                                                                    \
        TN_ISSUE(U, mc + (U) + TR_NSTAGE)                                                                                \
        if ((FULL || mc + (U) + 1 < nmc_run) && !no_frag) tr_read_asm<((U) + 1) & 3>(fa, fb, NXT);                       \
        TN_COMPUTE(CUR)                                                                                                  \
        if (PSA && first) tn_psa_chunk<(U)>(hold, tot_lds, wv, gbh, pq_hold, po_hold, lane);     /* behind the MFMAs' issue */   \
        if (!PSA && BRS && want_bias && --seg_left == 0) {                                                               \
            const float sc = brs[seg_sample];                                                                            \
            _Pragma("unroll") for (int j = 0; j < 4; ++j) { ctot[j] += sc * csum[j]; csum[j] = 0.f; }                    \
            seg_left = seg_stages; ++seg_sample;                                                                         \
        }                                                                                                                \
        if (PSA) {                                                                                                       \
            if ((U) == 3) {                                                                                              \
                first = false;                                                                                           \
                if (--seg_left == 0 && !(psa.dbg & 1)) {                                                                 \
                    tn_psa_begin(acc, hold, gacc, ctot, gbh, po_g, psa_g, brs, seg_sample, lane, z8);                    \
                    first = true; pq_hold = pq_row; po_hold = po_row;                                                    \
                    pq_row += 1024u; po_row += 1536u; po_g += 1536u; seg_left = seg_iters; ++seg_sample;                 \
                }                                                                                                        \
            }                                                                                                            \
        }                                                                                                                \
        tr_wait(NXT);                                                                                                    \
    }

    TN_ISSUE(0, 0) TN_ISSUE(1, 1) TN_ISSUE(2, 2) TN_ISSUE(3, 3)
    if constexpr (PSA) {
        // the coefficient / weight loads were issued before the first four stages' DMA and complete before it (loads return in order); the
        // values are pinned here — passing them through an empty asm keeps hipcc from putting their wait at the first use inside the
        // pipelined loop, where a vmcnt(0) would drain the operand DMA at every sample boundary
#pragma unroll
        for (int sidx = 0; sidx < TN_PSA_MAXS; ++sidx) pq_tab[sidx * 256 + tid] = tv[sidx];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(wv[i][j]));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    int mc = 0;
    if (nmc_run > 0) {
        // stage 0 landed: its 4 DMA are the oldest of up to 16
        if (nmc >= 4) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (!no_frag) tr_read_asm<0>(fa, fb, P);
        tr_wait(P);
#define TN_ITER(FULL, CH) TN_STEP(0, P, Q, FULL, CH) TN_STEP(1, Q, P, FULL, CH) TN_STEP(2, P, Q, FULL, CH) TN_STEP(3, Q, P, FULL, CH)
#define TN_CHUNKS tn_psa_chunk<0>(hold, tot_lds, wv, gbh, pq_hold, po_hold, lane); tn_psa_chunk<1>(hold, tot_lds, wv, gbh, pq_hold, po_hold, lane); \
                  tn_psa_chunk<2>(hold, tot_lds, wv, gbh, pq_hold, po_hold, lane); tn_psa_chunk<3>(hold, tot_lds, wv, gbh, pq_hold, po_hold, lane);
        for (; mc + 7 <= nmc_run; mc += 4) {          // steps mc .. mc+3 all have stages mc+U+3 <= nmc-1 behind them
            TN_ITER(true, false)                      // PSA: the four chunks of a parked sample ride in the sample's first four steps (a second
                                                      // copy of the loop body with unconditional chunks made hipcc spill 160 registers)
        }
        for (; mc < nmc_run; mc += 4) {
            TN_ITER(false, false)
        }
    }
#undef TN_ITER
#undef TN_STEP
#undef TN_COMPUTE
#undef TN_ISSUE
    if constexpr (PSA) {
        if (first) { TN_CHUNKS }          // the split's last sample was parked by the final step
    }
#undef TN_CHUNKS

    // ---- write this split's 128x128 partial to its fp32 slab: each wave transposes its 64x64 accumulator block through
    // a private LDS stage (two 32-row passes) so that every store instruction writes 4 rows x 256 contiguous bytes
    __syncthreads();                       // the ring is free
    if constexpr (PSA) {                   // the samples' statistics: LDS -> Rpart / G
        const int ns = nmc / seg_stages, b0 = m_beg / psa.T;
        for (int idx = tid; idx < ns * 384 && !(psa.dbg & 16); idx += 256) {
            const int sl = idx / 384, e = idx - sl * 384;
            const float v = psa_out[idx];
            if (e < 256) {
                const int w_ = e >> 6, row = e & 63;
                psa.Rpart[((size_t)(b0 + sl) * (Nb >> 6) + nt * 2 + (w_ & 1)) * Ka + k0 + (w_ >> 1) * 64 + row] = v;
            } else if (kt == 0) psa.G[(size_t)(b0 + sl) * Nb + n0 + (e - 256)] = v;
        }
    }
    if (DBG != 0 && (dbg & 8) != 0) { if (acc[0][0][0] == 123.f) out[0] = acc[1][1][1]; return; }
    {
        constexpr int SLD = 68;
        float* stage = reinterpret_cast<float*>(smem) + wid * (32 * SLD);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
#pragma unroll
            for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        stage[(16 * ii + 4 * (lane >> 4) + r) * SLD + 16 * j + (lane & 15)] = PSA ? tot_tab[(wid * 16 + (2 * p + ii) * 4 + j) * 64 + lane][r] : acc[2 * p + ii][j][r];
            float* orow = out + (size_t)split * sstride + (size_t)(k0 + wr * 64 + 32 * p + (lane >> 4)) * Nb + n0 + wc * 64 + (lane & 15) * 4;
#pragma unroll
            for (int it = 0; it < 8; ++it)       // one instruction = 4 rows x 256 contiguous bytes
                *reinterpret_cast<float4*>(orow + (size_t)(4 * it) * Nb) = *reinterpret_cast<const float4*>(stage + ((lane >> 4) + 4 * it) * SLD + (lane & 15) * 4);
        }
    }
    if (want_bias) {   // lane (g, c) holds the sum over rows 8g..8g+7 (mod 32) of column 16j + c: fold the 4 row groups
        if (PSA) {      // every sample of the split was folded at its boundary; all four row groups hold the full sums
#pragma unroll
            for (int j = 0; j < 4; ++j) csum[j] = (lane >> 4) == 0 ? ctot[j] : 0.f;
        } else if (BRS) {      // the rows of the last, unfinished sample of this split
            const float sc = seg_left != seg_stages && seg_sample * brsT < M ? brs[seg_sample] : 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) csum[j] = ctot[j] + sc * csum[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float t = csum[j];
            t += __shfl_xor(t, 16, 64);
            t += __shfl_xor(t, 32, 64);
            if (lane < 16) dbias[(size_t)split * sstride + n0 + wc * 64 + 16 * j + lane] = t;
        }
    }
    if (PSA && prev.nmain > 0 && prev.inl) {        // the previous launch's slab sums, a share per workgroup
        __syncthreads();
        tn_reduce_block(prev, (int)blockIdx.x, (int)gridDim.x, reinterpret_cast<float4 (*)[32]>(smem));
    }
}

static void tn_plan(int M, int Ka, int Nb, int dtM, int& splits, int& rows_per_split) {
    const int MC = dtM == DT_BF16 ? 64 : 32;
    const int tiles = ((Ka + 127) / 128) * ((Nb + 127) / 128);
    int want = (768 + tiles - 1) / tiles;                 // ~3 workgroups per CU
    const int maxs = (M + 4 * MC - 1) / (4 * MC);         // at least 4 LDS tiles per split
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    rows_per_split = ((M + want - 1) / want + MC - 1) / MC * MC;
    splits = (M + rows_per_split - 1) / rows_per_split;
}

size_t gemm_tn_slab_floats(int M, int Ka, int Nb, int dtM) {
    int splits, rps;
    tn_plan(M, Ka, Nb, dtM, splits, rps);
    if (splits < 512) splits = 512;        // the transposed-read kernel plans <= 512 splits
    return (size_t)splits * ((size_t)Ka * Nb + Nb);
}

int g_force_tn_regstage = 0;   // tests: force the register-transposing TN kernel
int g_dbg_tn = 0;           // ablation bits for the TN kernel: 1 skip MFMA, 2 skip LDS stores, 4 skip global loads

int g_tn_blocks = 0;
int g_tn_phase = 0;            // 0: GEMM + slab sums; 1: GEMM kernel only; 2: slab sums only (the model profiles the two separately)

// PSA split plan: whole samples per split (the statistics of a sample come from one workgroup per output tile), at most TN_PSA_MAXS of them,
// as close to one workgroup per CU as the batch allows; 0 = no such plan
static int tn_psa_splits(int M, int Ka, int Nb, int T) {
    if (T <= 0 || T % (4 * TR_ROWS) != 0 || M % T != 0) return 0;      // samples = whole iterations of the 4x unrolled step loop
    const int Bn = M / T, tiles = (Ka / 128) * (Nb / 128);
    const int want = max(1, 256 / tiles);
    for (int d = min(want, Bn); d >= 1; --d) {
        if (Bn % d != 0) continue;
        if (d > 8 && (d & 7) != 0) continue;              // keeps the XCD-aware (tile, split) mapping
        const int ns = Bn / d;
        if (ns > TN_PSA_MAXS) return 0;
        if (ns * T < 256) continue;                       // at least 8 stages per split
        return d;
    }
    return 0;
}
// the bf16 transposed-read kernels take this shape (whole 128 x 128 tiles, whole 32-row stages, at least 8 of them); every test of it reads this
static bool tn_tr_takes(int dtA, int dtB, int dtM, int M, int Ka, int Nb) {
    return dtA == DT_BF16 && dtB == DT_BF16 && dtM == DT_BF16 && M % 64 == 0 && Ka % 128 == 0 && Nb % 128 == 0 && M >= 256 && !g_force_tn_regstage;
}
bool gemm_tn_psa_ok(int dtA, int dtB, int dtM, int M, int Ka, int Nb, int T) {
    return tn_tr_takes(dtA, dtB, dtM, M, Ka, Nb) && !g_dbg_tn && tn_psa_splits(M, Ka, Nb, T) > 0;
}

// split plan of the plain and the weighted-bias-sum transposed-read kernel: M-splits and rows per split (whole 32-row stages, at least 8 per split
// where M allows)
static void tn_tr_plan(int M, int Ka, int Nb, int& splits, int& rps) {
    const int tiles = (Ka / 128) * (Nb / 128);
    // workgroups: one per CU for up to 8 tiles (same kernel time as two per CU, half the slab bytes: the slab sums go
    // 9.6 -> 7.3 us), two per CU for 12+ tiles (N = 768: 61 vs 72 us); g_tn_blocks != 0 overrides (tools/tn_ablate.py)
    const int blocks = g_tn_blocks ? g_tn_blocks : (tiles <= 8 ? 256 : 512);
    int want = max(1, blocks / tiles);
    const int maxs = max(1, M / 256);                     // at least 8 tiles per split
    if (want > maxs) want = maxs;
    if (want > 8) want &= ~7;                             // a multiple of 8 keeps the XCD-aware (tile, split) mapping: 12 tiles x 42 splits ran 102 us, x 40: see DESIGN.md
    rps = ((M + want - 1) / want + TR_ROWS - 1) / TR_ROWS * TR_ROWS;
    splits = (M + rps - 1) / rps;
    while (want > 8 && (splits & 7) != 0 && rps > TR_ROWS) { rps -= TR_ROWS; splits = (M + rps - 1) / rps; if (splits > 512) break; }
    if (splits > 512) { rps = ((M + want - 1) / want + TR_ROWS - 1) / TR_ROWS * TR_ROWS; splits = (M + rps - 1) / rps; }
}

// the transposed-read kernels: plan.route is TN_BIG, TN_TR, TN_TR_BRS or TN_TR_PSA
static int run_tn_tr(const TnPlan& plan, const void* A, const void* B, float* out, float* dbias, float* slab, int M, int Ka, int Nb, hipStream_t s, int ka_valid, int nb_valid,
                     const float* brs, int brsT, TnDefer* defer, const TnPsa* psa) {
    if (plan.route == TN_BIG) {
        // config #4's shapes (Ka, Nb >= 512 in whole 256-wide tiles, M >= 32768): the 256 x 256 tile kernel of gemm_big.hip, sums right behind it
        int bsplits = plan.splits;
        launch_gemm_tn_flush(defer, s);
        if (g_tn_phase != 2) {
            const int rc = launch_gemm_tn_big(A, B, slab, dbias ? 1 : 0, M, Ka, Nb, &bsplits, (brs && dbias) ? brs : nullptr, brsT, s);
            if (rc == 1) { ishara_set_error("gemm_tn: internal error: the kernel gemm_tn_route chose refused the call (M=%d Ka=%d Nb=%d)", M, Ka, Nb); return -2; }
            if (rc != 0) return rc;
        }
        if (g_tn_phase != 1) launch_reduce_slabs2(slab, out, Ka * Nb, dbias, dbias ? Nb : 0, bsplits, (size_t)Ka * Nb + Nb, s, 0, 0);
        return launch_rc();
    }
    const int tiles = (Ka / 128) * (Nb / 128);
    const TnPsa nopsa = {};
    const int splits = plan.splits, rps = plan.rps;
    if (splits <= 0 || rps <= 0) { ishara_set_error("gemm_tn: internal error: no split plan for the route gemm_tn_route chose (M=%d Ka=%d Nb=%d)", M, Ka, Nb); return -2; }
    if (defer && g_tn_phase == 0 && !g_dbg_tn && tiles * splits > 256 && !psa) {
        // a launch that fills the chip twice over (12+ tiles at two workgroups per CU) neither carries riders nor defers its own sums: the riders
        // would queue behind 512 workgroups and its slabs (2 MB x 16 splits for a 1024 x 512 weight) make the next launch's riders the tail
        // (configs[3]: 47.9 -> 51.5 ms/step with the deferral on everywhere)
        launch_gemm_tn_flush(defer, s);
        defer = nullptr;
    }
    if (defer && g_tn_phase == 0 && !g_dbg_tn) {
        // deferred sums: this launch writes the slab buffer whose turn it is, and carries the sums of the previous launch's slabs
        slab = defer->slab[defer->turn];
        float* bias_slab2 = dbias ? slab + (size_t)Ka * Nb : nullptr;
        TnRed prev = {};
        const int nmain = tiles * splits;
        int riders = 0;
        if (defer->pending) {
            prev = TnRed{defer->p_slab, defer->p_out0, defer->p_out1, defer->p_n0, defer->p_n, defer->p_splits, defer->p_stride, defer->p_nb, defer->p_nbv, nmain, psa ? 1 : 0};
            riders = psa ? 0 : min(128, (defer->p_n + 127) / 128);
        }
        const dim3 grid(nmain + riders);
        if (psa) hipLaunchKernelGGL((gemm_tn_tr_kernel<0, false, true>), grid, dim3(256), 0, s, (const bf16*)A, (const bf16*)B, slab, bias_slab2, M, Ka, Nb, rps, tiles, splits, 0, brs, brsT, prev, *psa);
        else if (brs && bias_slab2) hipLaunchKernelGGL((gemm_tn_tr_kernel<0, true>), grid, dim3(256), 0, s, (const bf16*)A, (const bf16*)B, slab, bias_slab2, M, Ka, Nb, rps, tiles, splits, 0, brs, brsT, prev, nopsa);
        else hipLaunchKernelGGL((gemm_tn_tr_kernel<0, false>), grid, dim3(256), 0, s, (const bf16*)A, (const bf16*)B, slab, bias_slab2, M, Ka, Nb, rps, tiles, splits, 0, brs, brsT, prev, nopsa);
        const size_t stride = (size_t)Ka * Nb + Nb;
        const int n0 = ka_valid * Nb, n1 = dbias ? Nb : 0;
        if (!reduce_cols_ok(slab, out, dbias, n0, n0 + n1, stride) || splits > 64) {        // shapes the rider layout does not take: sum now
            launch_reduce_slabs2(slab, out, n0, dbias, n1, splits, stride, s, nb_valid ? Nb : 0, nb_valid);
            defer->pending = false;
        } else {
            defer->pending = true;
            defer->p_slab = slab; defer->p_out0 = out; defer->p_out1 = dbias; defer->p_n0 = n0; defer->p_n = n0 + n1; defer->p_splits = splits; defer->p_stride = stride;
            defer->p_nb = nb_valid ? Nb : 0; defer->p_nbv = nb_valid;
        }
        defer->turn ^= 1;
        return launch_rc();
    }
    float* bias_slab = dbias ? slab + (size_t)Ka * Nb : nullptr;        // bias partials sit right behind each split's weight partial
    const TnRed noprev = {};
    if (g_tn_phase != 2)
    {
        if (psa) hipLaunchKernelGGL((gemm_tn_tr_kernel<0, false, true>), dim3(tiles * splits), dim3(256), 0, s, (const bf16*)A, (const bf16*)B, slab, bias_slab, M, Ka, Nb, rps, tiles, splits, 0, brs, brsT, noprev, *psa);
        else if (g_dbg_tn) hipLaunchKernelGGL((gemm_tn_tr_kernel<1, false>), dim3(tiles * splits), dim3(256), 0, s, (const bf16*)A, (const bf16*)B, slab, bias_slab, M, Ka, Nb, rps, tiles, splits, g_dbg_tn, brs, brsT, noprev, nopsa);
        else if (brs && bias_slab) hipLaunchKernelGGL((gemm_tn_tr_kernel<0, true>), dim3(tiles * splits), dim3(256), 0, s, (const bf16*)A, (const bf16*)B, slab, bias_slab, M, Ka, Nb, rps, tiles, splits, 0, brs, brsT, noprev, nopsa);
        else hipLaunchKernelGGL((gemm_tn_tr_kernel<0, false>), dim3(tiles * splits), dim3(256), 0, s, (const bf16*)A, (const bf16*)B, slab, bias_slab, M, Ka, Nb, rps, tiles, splits, 0, brs, brsT, noprev, nopsa);
    }
    if (g_tn_phase != 1)
        launch_reduce_slabs2(slab, out, ka_valid * Nb, dbias, dbias ? Nb : 0, splits, (size_t)Ka * Nb + Nb, s, nb_valid ? Nb : 0, nb_valid);   // rows >= ka_valid of A / columns >= nb_valid of B are zero padding
    return launch_rc();
}

template <typename TA, typename TB, typename TM>
static int run_tn(const TnPlan& plan, int opA, int opB, const void* A, const void* B, float* out, float* dbias, float* slab,
                  int M, int Ka, int Nb, const OpArgs& oa, const OpArgs& ob, hipStream_t s) {
    const int splits = plan.splits, rps = plan.rps;
    float* bias_slab = dbias ? slab + (size_t)splits * Ka * Nb : nullptr;
    const int tiles = ((Ka + 127) / 128) * ((Nb + 127) / 128);
    const int a_ok = (((size_t)Ka * sizeof(TA)) % 16 == 0) && (((uintptr_t)A) % 16 == 0);
    const int b_ok = (((size_t)Nb * sizeof(TB)) % 16 == 0) && (((uintptr_t)B) % 16 == 0);
    if (g_tn_phase != 2)
        hipLaunchKernelGGL((gemm_tn_kernel<TA, TB, TM>), dim3(tiles, splits), dim3(256), 0, s,
                           (const TA*)A, (const TB*)B, slab, bias_slab, M, Ka, Nb, rps, a_ok, b_ok, opA, opB, oa, ob, g_dbg_tn);
    if (g_tn_phase != 1) {
        launch_reduce_slabs(slab, out, Ka * Nb, splits, (size_t)Ka * Nb, s);
        if (dbias) launch_reduce_slabs(bias_slab, dbias, Nb, splits, (size_t)Nb, s);
    }
    return launch_rc();
}

// sums whatever slabs a deferring caller still has pending (end of the backward pass, or before the gradient is read)
int launch_gemm_tn_flush(TnDefer* defer, hipStream_t s) {
    if (defer && defer->pending) {
        launch_reduce_slabs2(defer->p_slab, defer->p_out0, defer->p_n0, defer->p_out1, defer->p_n - defer->p_n0, defer->p_splits, defer->p_stride, s, defer->p_nb, defer->p_nbv);
        defer->pending = false;
    }
    return launch_rc();
}

bool gemm_tn_bias_rowscale_ok(int dtA, int dtB, int dtM, int M, int Ka, int Nb, int T) {
    return tn_tr_takes(dtA, dtB, dtM, M, Ka, Nb) && T > 0 && T % 32 == 0;
}

// The kernel a call runs on, decided here and nowhere else: launch_gemm_tn launches what this returns and gemm_tn_kernel_name names it.
// ka_valid / nb_valid as the caller passes them (0: no padding); brs / psa: the call has a bias row scale / a TnPsa, with their T.
TnRoute gemm_tn_route(int dtA, int dtB, int dtM, int opA, int opB, int M, int Ka, int Nb, int ka_valid, int nb_valid, bool brs, int brsT, bool psa, int psaT) {
    if (psa && (!gemm_tn_psa_ok(dtA, dtB, dtM, M, Ka, Nb, psaT) || opA != OP_NONE || opB != OP_NONE || ka_valid > 0 || nb_valid > 0 || (brs && brsT != psaT))) return TN_REFUSED;
    if (ka_valid <= 0) ka_valid = Ka;
    if (nb_valid >= Nb || nb_valid < 0) nb_valid = 0;
    if (brs && !gemm_tn_bias_rowscale_ok(dtA, dtB, dtM, M, Ka, Nb, brsT)) return TN_REFUSED;
    if (dtA == DT_F32 && dtB == DT_F32 && dtM == DT_F32) return TN_REG;
    if (tn_tr_takes(dtA, dtB, dtM, M, Ka, Nb) && opA == OP_NONE && opB == OP_NONE) {
        if (psa) return TN_TR_PSA;
        int bs = 0;       // the 256 x 256 tile kernel (gemm_big.hip) takes a bias row scale only with T % 128 == 0
        if ((!brs || (brsT > 0 && brsT % 128 == 0)) && !g_dbg_tn && !g_tn_blocks && ka_valid == Ka && !nb_valid && gemm_tn_big_plan(M, Ka, Nb, &bs) > 0) return TN_BIG;
        return brs ? TN_TR_BRS : TN_TR;
    }
    if (ka_valid != Ka || nb_valid) return TN_REFUSED;         // padded operands: the transposed-read kernel only
    return dtM == DT_BF16 && (dtA == DT_BF16 || dtA == DT_F32) && (dtB == DT_BF16 || dtB == DT_F32) && !(dtA == DT_F32 && dtB == DT_F32) ? TN_REG : TN_REFUSED;
}

// What launch_gemm_tn does with a call, decided here and nowhere else: every refusal with its message (route TN_REFUSED), else the route and the
// split plan the launch uses.  Host only; A / B: the operand addresses (their alignment is checked, nothing is read)
TnPlan gemm_tn_plan(int dtA, int dtB, int dtM, int opA, int opB, const void* A, const void* B, bool has_dbias, int M, int Ka, int Nb,
                    int ka_valid, int nb_valid, const float* bias_rowscale, int bias_T, const TnPsa* psa) {
    const TnPlan refused = {TN_REFUSED, 0, 0};
    if (M <= 0 || Ka <= 0 || Nb <= 0) { ishara_set_error("gemm_tn: bad shape"); return refused; }
    const TnRoute route = gemm_tn_route(dtA, dtB, dtM, opA, opB, M, Ka, Nb, ka_valid, nb_valid, bias_rowscale != nullptr, bias_T, psa != nullptr, psa ? psa->T : 0);
    if (psa && (route != TN_TR_PSA || !psa->P || !psa->Q || !psa->W || !psa->G || !psa->Rpart)) {
        ishara_set_error("gemm_tn: per-sample affine needs the transposed-read kernel, whole samples per split and all of P, Q, W, G, Rpart (gemm_tn_psa_ok)"); return refused;
    }
    if (bias_rowscale && !gemm_tn_bias_rowscale_ok(dtA, dtB, dtM, M, Ka, Nb, bias_T)) { ishara_set_error("gemm_tn: bias row scale needs the transposed-read kernel and T %% 32 == 0"); return refused; }
    if (ka_valid <= 0) ka_valid = Ka;
    if (nb_valid >= Nb || nb_valid < 0) nb_valid = 0;
    if (nb_valid % 4 != 0) { ishara_set_error("gemm_tn: nb_valid %d must be a multiple of 4", nb_valid); return refused; }
    if ((dtA == DT_BF16 && Ka % 8 != 0) || (dtA == DT_F32 && Ka % 4 != 0) || (dtB == DT_BF16 && Nb % 8 != 0) || (dtB == DT_F32 && Nb % 4 != 0) ||
        ((uintptr_t)A) % 16 != 0 || ((uintptr_t)B) % 16 != 0) {
        ishara_set_error("gemm_tn: operand rows must be 16-byte aligned (Ka=%d Nb=%d)", Ka, Nb); return refused;
    }
    TnPlan p = {route, 0, 0};
    switch (route) {
        case TN_REFUSED:
            if (ka_valid != Ka || nb_valid) ishara_set_error("gemm_tn: padded A columns need the bf16 transposed-read kernel (M %% 64, Ka %% 128, Nb %% 128)");
            else ishara_set_error("gemm_tn: unsupported dtype combination %d/%d/%d", dtA, dtB, dtM);
            return refused;
        case TN_BIG: case TN_TR: case TN_TR_BRS: case TN_TR_PSA:
            if (ka_valid < Ka && has_dbias) { ishara_set_error("gemm_tn: padded A columns with a bias gradient"); return refused; }
            if (route == TN_BIG) p.rps = gemm_tn_big_plan(M, Ka, Nb, &p.splits);
            else if (route == TN_TR_PSA) { p.splits = tn_psa_splits(M, Ka, Nb, psa->T); p.rps = p.splits > 0 ? M / p.splits : 0; }
            else tn_tr_plan(M, Ka, Nb, p.splits, p.rps);
            break;
        case TN_REG:
            tn_plan(M, Ka, Nb, dtM, p.splits, p.rps);
            break;
    }
    return p;
}

int launch_gemm_tn(int dtA, int dtB, int dtM, int opA, int opB, const void* A, const void* B,
                   float* out, float* dbias, float* slab, int M, int Ka, int Nb,
                   const OpArgs& oa, const OpArgs& ob, hipStream_t s, int ka_valid, int nb_valid, const float* bias_rowscale, int bias_T, TnDefer* defer, const TnPsa* psa) {
    const TnPlan plan = gemm_tn_plan(dtA, dtB, dtM, opA, opB, A, B, dbias != nullptr, M, Ka, Nb, ka_valid, nb_valid, bias_rowscale, bias_T, psa);
    if (ka_valid <= 0) ka_valid = Ka;
    if (nb_valid >= Nb || nb_valid < 0) nb_valid = 0;
    switch (plan.route) {
        case TN_REFUSED:
            return -1;
        case TN_BIG: case TN_TR: case TN_TR_BRS: case TN_TR_PSA:
            return run_tn_tr(plan, A, B, out, dbias, slab, M, Ka, Nb, s, ka_valid, nb_valid, bias_rowscale, bias_T, defer, psa);
        case TN_REG:
            if (dtM == DT_F32) return run_tn<float, float, float>(plan, opA, opB, A, B, out, dbias, slab, M, Ka, Nb, oa, ob, s);
            if (dtA == DT_F32) return run_tn<float, bf16, bf16>(plan, opA, opB, A, B, out, dbias, slab, M, Ka, Nb, oa, ob, s);
            if (dtB == DT_F32) return run_tn<bf16, float, bf16>(plan, opA, opB, A, B, out, dbias, slab, M, Ka, Nb, oa, ob, s);
            return run_tn<bf16, bf16, bf16>(plan, opA, opB, A, B, out, dbias, slab, M, Ka, Nb, oa, ob, s);
    }
    return -1;
}

// profiler key = the prefix of the rocprof name of the kernel launch_gemm_tn launches for the same arguments
const char* gemm_tn_kernel_name(int dtA, int dtB, int dtM, int opA, int opB, int M, int Ka, int Nb, int ka_valid, int nb_valid, const float* bias_rowscale, int bias_T, const TnPsa* psa) {
    switch (gemm_tn_route(dtA, dtB, dtM, opA, opB, M, Ka, Nb, ka_valid, nb_valid, bias_rowscale != nullptr, bias_T, psa != nullptr, psa ? psa->T : 0)) {
        case TN_BIG: return "gemm_tn_big_kernel";
        case TN_TR: case TN_TR_BRS: return "gemm_tn_tr_kernel<0>";          // one key for the plain and the weighted-bias-sum instantiation
        case TN_TR_PSA: return "gemm_tn_tr_kernel<0,false,true>";           // its own key: this instantiation does the statistics pass's work too
        default: break;           // TN_REG, and TN_REFUSED (nothing runs): the register-transposing kernel of the types
    }
    return dtM == DT_F32 ? "gemm_tn_kernel<f32,f32,f32>" : (dtA == DT_F32 ? "gemm_tn_kernel<f32,bf16,bf16>" : (dtB == DT_F32 ? "gemm_tn_kernel<bf16,f32,bf16>" : "gemm_tn_kernel<bf16,bf16,bf16>"));
}
