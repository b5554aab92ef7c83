// MFMA GEMMs for the dense projections of the Ishara encoder (gfx950 / CDNA4).
//
//   gemm_nt : C[M,N]  = epi( op(A)[M,K] . Bt[N,K]^T )       forward + dgrad   (this file: the tile kernels, the kernel route, launcher, profiler key)
//   gemm_tn : dW[K,N] += opA(A)[M,K]^T . opB(B)[M,N]         wgrad (+ bias grad), split over M   (gemm_tn.hip; slab sums in reduce.hip)
//
// M = batch*frames is huge (98,304 for B256,T384) while N,K <= 768, so both kernels
// stream the activation operand once from HBM and keep the weight tile L2-resident.
// One 256-thread workgroup (4 waves, 2x2) owns a 128x128 output tile; each wave a 64x64
// sub-tile = 4x4 MFMA 16x16 accumulators.  bf16 mode uses v_mfma_f32_16x16x32_bf16,
// f32 mode uses the exact-f32 v_mfma_f32_16x16x4_f32 (same tile structure, K tile is
// 128 bytes per row in both: 64 bf16 / 32 f32).  Operands are register-staged
// (global -> VGPR -> transform -> LDS, issue-early/write-late) into a double-buffered,
// XOR-swizzled LDS image; the accumulators leave through an fp32 LDS stage so that
// the fused epilogue (bias, PE table, activation, dropout, drop-path, act', residual,
// QKV head split with V transposed) runs on whole 8-element row chunks with 16-byte
// coalesced global accesses.
#include "gemm_tile.h"

// ---------------------------------------------------------------------------------
// NT kernel
// ---------------------------------------------------------------------------------
template <typename TA, typename TM, typename TC, int OP>
__global__ __launch_bounds__(256) void gemm_nt_kernel(const TA* __restrict__ A, const TM* __restrict__ Bt, TC* __restrict__ C,
                                                      int M, int N, int K, int ldb, int a_vec_ok, OpArgs oa, EpiArgs ea) {
    __shared__ __attribute__((aligned(16))) char smem[65536];
    constexpr int BK = MmaCfg<TM>::BK;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
    const int nMt = (M + 127) >> 7, nNt = (N + 127) >> 7;
    int mt, nt;
    {   // XCD-aware mapping: blocks b, b+8 share an XCD (L2); keep one A row-panel's N tiles together
        const int id = blockIdx.x;
        if ((nMt & 7) == 0) { const int xcd = id & 7, local = id >> 3; mt = (local / nNt) * 8 + xcd; nt = local % nNt; }
        else { mt = id / nNt; nt = id % nNt; }
    }
    const int m0 = mt << 7, n0 = nt << 7;
    const int nk = (K + BK - 1) / BK;

    u32x4 ra[4], rb[4];
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    nt_gload<TA, TM, OP>(A, Bt, M, K, ldb, a_vec_ok != 0, m0, n0, 0, tid, oa, ra, rb);
    nt_lstore(smem, tid, ra, rb);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) nt_gload<TA, TM, OP>(A, Bt, M, K, ldb, a_vec_ok != 0, m0, n0, kt + 1, tid, oa, ra, rb);
        const char* sa = smem + (kt & 1) * 32768;
        mma_tile<TM, 0>(sa, sa + 16384, wr, wc, lane, acc);
        if (more) nt_lstore(smem + ((kt + 1) & 1) * 32768, tid, ra, rb);
        __syncthreads();
    }

    // ---- epilogue through an fp32 LDS stage, 64 rows per pass ----
    float* stage = reinterpret_cast<float*>(smem);   // [64][132]
    constexpr int SLD = 132;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        EpiRows<TC, 4> er;       // thread -> columns (tid&15)*8.., rows (tid>>4) + 16q of this 64-row pass
        er.prefetch(m0 + 64 * p + (tid >> 4), 16, n0 + (tid & 15) * 8, M, N, ea);
        if (wr == p) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        stage[(16 * i + 4 * (lane >> 4) + r) * SLD + wc * 64 + 16 * j + (lane & 15)] = acc[i][j][r];
        }
        __syncthreads();
        er.finish(stage + (tid >> 4) * SLD + (tid & 15) * 8, 16 * SLD, M, N, ea, C);
        if (ea.mode == EPI_QKV) {   // V columns: write transposed vt[b,h,i,t], 8 consecutive t per store
            const int d = ea.H * ea.dh;
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                const int c = tid + 256 * qq, col = c & 127, rg = c >> 7;
                const int n = n0 + col, mb = m0 + 64 * p + 8 * rg;
                if (n < N && mb < M) {
                    int h, part, i;
                    if (ea.head_major) { h = n / (3 * ea.dh); const int w = n - h * 3 * ea.dh; part = w / ea.dh; i = w - part * ea.dh; }
                    else { part = n / d; const int w = n - part * d; h = w / ea.dh; i = w - h * ea.dh; }
                    if (part == 2) {
                        float v[8];
                        const float bias = ea.bias ? ea.bias[n] : 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = stage[(8 * rg + e) * SLD + col] + bias;
                        const int b = mb / ea.T, t = mb - b * ea.T;
                        TC* dst = reinterpret_cast<TC*>(ea.vt) + ((size_t)(b * ea.H + h) * ea.dh + i) * ea.T + t;
                        store8_n(dst, v, min(8, M - mb));
                    }
                }
            }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------
// NT kernel, LDS-DMA pipelined (the common case: A and Bt both of the MFMA type, no operand
// transform, K a multiple of the K tile).  Tile 64(M) x 128(N); 4 waves (2x2), wave tile
// 32x64 = 2x4 MFMA 16x16.  A 3-deep LDS ring is filled by global_load_lds_dwordx4 — no VGPR
// staging, no ds_write; the XOR swizzle is applied to the per-lane SOURCE address because
// the LDS side of an LDS-DMA is lane-linear — so two K tiles stay in flight while a third is
// consumed: one raw s_barrier and one counted s_waitcnt vmcnt(6) per K tile.  Each wave then
// drains its accumulators through a private fp32 LDS stage (no block barrier) into the fused
// epilogue with 16-byte coalesced stores.
// ---------------------------------------------------------------------------------
#define GL_STAGE 12288          // A 64 rows x 64 B + B 128 rows x 64 B   (K tile = 32 bf16 / 16 f32)
#define GL_NSTAGE 4
DEVI int gl_f(int row) { return ((row >> 3) & 1) << 1; }      // conflict-free slot swizzle for 64-byte rows (brute-forced)

// per-lane state of the LDS-DMA NT kernel: everything the K loop needs is computed once; per K tile the loop only
// bumps three global pointers by one tile and uses compile-time stage offsets (the loop is unrolled over the ring)
template <typename TM>
struct GlState {
    const TM* pa;            // this lane's 16-byte source of the A piece (row clamp + swizzle applied)
    const TM* pb[2];         // ... of the two B pieces
    int offA[2], offB[4];    // byte offsets of the MFMA fragment reads inside a stage (k-step 0)
};

template <typename TM>
DEVI void gl_init(GlState<TM>& g, const TM* __restrict__ A, const TM* __restrict__ Bt, int M, int K, int ldb, int m0, int n0,
                  int wid, int wr, int wc, int lane) {
    constexpr int EPC = MmaCfg<TM>::EPC;
    const int r = lane >> 2, sp = lane & 3;
    const int kcol = (sp ^ gl_f(r)) * EPC;
    g.pa = A + (size_t)min(m0 + 16 * wid + r, M - 1) * K + kcol;
#pragma unroll
    for (int u = 0; u < 2; ++u) g.pb[u] = Bt + (size_t)(n0 + 16 * (wid + 4 * u) + r) * ldb + kcol;
    const int fr = lane & 15, fg = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i) { const int row = wr * 32 + 16 * i + fr; g.offA[i] = row * 64 + (is_bf16_t<TM>::value ? ((fg ^ gl_f(row)) << 4) : (gl_f(row) << 4) + fg * 4); }
#pragma unroll
    for (int j = 0; j < 4; ++j) { const int row = wc * 64 + 16 * j + fr; g.offB[j] = 4096 + row * 64 + (is_bf16_t<TM>::value ? ((fg ^ gl_f(row)) << 4) : (gl_f(row) << 4) + fg * 4); }
}

template <typename TM>
DEVI void gl_issue(GlState<TM>& g, char* stage, int wid) {
    constexpr int BKH = MmaCfg<TM>::BK / 2;
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g.pa,
                                     (__attribute__((address_space(3))) void*)(stage + wid * 1024), 16, 0, 0);
#pragma unroll
    for (int u = 0; u < 2; ++u)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g.pb[u],
                                         (__attribute__((address_space(3))) void*)(stage + 4096 + (wid + 4 * u) * 1024), 16, 0, 0);
    g.pa += BKH; g.pb[0] += BKH; g.pb[1] += BKH;
}

template <typename TM>
DEVI void gl_mma(const GlState<TM>& g, const char* st, f32x4 (&acc)[2][4]) {
    if constexpr (is_bf16_t<TM>::value) {
        bf16x8 a[2], b[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const bf16x8*>(st + g.offA[i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const bf16x8*>(st + g.offB[j]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {          // f32: 4 k-steps of 4 per 64-byte row; slot s -> physical slot s ^ f(row): XOR the precomputed f-slot
            float a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const float*>(st + (g.offA[i] ^ (s << 4)));
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const float*>(st + (g.offB[j] ^ (s << 4)));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
}

template <typename TM, typename TC>
__global__ __launch_bounds__(256, 3) void gemm_nt_glds_kernel(const TM* __restrict__ A, const TM* __restrict__ Bt, TC* __restrict__ C,
                                                           int M, int N, int K, int ldb, EpiArgs ea) {
    __shared__ __attribute__((aligned(16))) char smem[GL_NSTAGE * GL_STAGE];
    constexpr int BK = MmaCfg<TM>::BK / 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    const int nMt = (M + 63) >> 6, nNt = (N + 127) >> 7;
    int mt, nt;
    {
        const int id = blockIdx.x;
        if ((nMt & 7) == 0) { const int xcd = id & 7, local = id >> 3; mt = (local / nNt) * 8 + xcd; nt = local % nNt; }
        else { mt = id / nNt; nt = id % nNt; }
    }
    const int m0 = mt << 6, n0 = nt << 7;
    const int nk = K / BK;

    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const bool ld_on = !(ea.dbg & 4), mma_on = !(ea.dbg & 2);
    // epilogue operands (bias, residual, act' input, drop-path scale) are requested first: their latency hides under the K loop
    const int mw = m0 + wr * 32, nw = n0 + wc * 64;
    EpiRows<TC, 4> er;       // thread -> columns (lane&7)*8.., rows (lane>>3) + 8q
    er.prefetch(mw + (lane >> 3), 8, nw + (lane & 7) * 8, M, N, ea);
    GlState<TM> gs;
    gl_init<TM>(gs, A, Bt, M, K, ldb, m0, n0, wid, wr, wc, lane);
#pragma unroll
    for (int st = 0; st < GL_NSTAGE - 1; ++st)
        if (st < nk && ld_on) gl_issue<TM>(gs, smem + st * GL_STAGE, wid);
    for (int kt0 = 0; kt0 < nk; kt0 += GL_NSTAGE) {
#pragma unroll
        for (int u = 0; u < GL_NSTAGE; ++u) {      // stage index u is a compile-time constant: LDS offsets fold into the instructions
            const int kt = kt0 + u;
            if (kt < nk) {
                // 3 DMA per wave per K tile; up to two later tiles stay in flight across the barrier
                const int ahead = min(nk - 1 - kt, GL_NSTAGE - 2);
                if (ahead >= 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
                else if (ahead == 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();          // tile kt landed for every wave; tile kt-1 fully consumed
                if (kt + GL_NSTAGE - 1 < nk && ld_on) gl_issue<TM>(gs, smem + ((u + GL_NSTAGE - 1) % GL_NSTAGE) * GL_STAGE, wid);
                if (mma_on) gl_mma<TM>(gs, smem + u * GL_STAGE, acc);
            }
        }
    }
    __syncthreads();     // ring is free: reuse it as four wave-private fp32 stages
    if (ea.dbg & 1) { if (acc[0][0][0] == 123.456f) C[0] = from_f<TC>(acc[1][3][2]); return; }

    constexpr int SLD = 68;
    float* stage = reinterpret_cast<float*>(smem) + wid * (32 * SLD);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                stage[(16 * i + 4 * (lane >> 4) + r) * SLD + 16 * j + (lane & 15)] = acc[i][j][r];
    er.finish(stage + (lane >> 3) * SLD + (lane & 7) * 8, 8 * SLD, M, N, ea, C);
    if (ea.mode == EPI_QKV) {
        const int d = ea.H * ea.dh;
        const int n = nw + lane;
        if (n < N) {
            int h, part, i;
            if (ea.head_major) { h = n / (3 * ea.dh); const int w = n - h * 3 * ea.dh; part = w / ea.dh; i = w - part * ea.dh; }
            else { part = n / d; const int w = n - part * d; h = w / ea.dh; i = w - h * ea.dh; }
            if (part == 2) {
                const float bias = ea.bias ? ea.bias[n] : 0.f;
#pragma unroll
                for (int rg = 0; rg < 4; ++rg) {
                    const int mb = mw + 8 * rg;
                    if (mb < M) {
                        float v[8];
#pragma unroll
                        for (int e = 0; e < 8; ++e) v[e] = stage[(8 * rg + e) * SLD + lane] + bias;
                        const int b = mb / ea.T, t = mb - b * ea.T;
                        TC* dst = reinterpret_cast<TC*>(ea.vt) + ((size_t)(b * ea.H + h) * ea.dh + i) * ea.T + t;
                        store8_n(dst, v, min(8, M - mb));
                    }
                }
            }
        }
    }
}

template <typename TM, typename TC>
static int run_nt_glds(const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const EpiArgs& ea, hipStream_t s) {
    const int nMt = (M + 63) / 64, nNt = (N + 127) / 128;
    hipLaunchKernelGGL((gemm_nt_glds_kernel<TM, TC>), dim3(nMt * nNt), dim3(256), 0, s, (const TM*)A, (const TM*)Bt, (TC*)C, M, N, K, ldb, ea);
    return launch_rc();
}

// ---------------------------------------------------------------------------------
// NT kernel v2 ("T"): 128x128 tile, LDS-DMA ring of 3 x 16 KB (K tile 32 bf16 / 16 f32, 64-byte rows), 4 waves (2x2),
// wave tile 64x64 held TRANSPOSED: acc[j][i] = mfma(Bt fragment, A fragment) so that a lane owns, for row
// m = 16i + (lane&15), the 4 CONSECUTIVE output columns n = 16j + 4*(lane>>4) .. +3.  The epilogue therefore runs
// straight from the accumulators — 8-byte (bf16) / 16-byte (f32) loads of residual / act' operands and stores of C per
// lane, no LDS staging, no block barrier — and the weight tile is re-read from L2 half as often as with 64-row tiles.
// ---------------------------------------------------------------------------------
#define GT_STAGE 16384
#define GT_NSTAGE 3

template <typename TM>
struct GtState {
    const TM* pa[2];
    const TM* pb[2];
    int offA[4], offB[4];
};

template <typename T> DEVI void load4t(const T* p, float (&v)[4]) { load4g(p, v); }
template <typename T> DEVI void store4t(T* p, const float (&v)[4]) { store4(p, v); }

// EK: 0 generic run-time-flag epilogue; 1 fast "C = acc + bias"; 2 fast "C = acc + bias + resid" (the epilogue is
// instruction-issue bound: the generic one costs ~800 instructions per wave-tile, the fast ones ~150)
template <typename TM, typename TC, int EK>
__global__ __launch_bounds__(256, 3) void gemm_nt_t_kernel(const TM* __restrict__ A, const TM* __restrict__ Bt, TC* __restrict__ C,
                                                           int M, int N, int K, int ldb, EpiArgs ea) {
    __shared__ __attribute__((aligned(16))) char smem[GT_NSTAGE * GT_STAGE];
    constexpr int EPC = MmaCfg<TM>::EPC, BK = MmaCfg<TM>::BK / 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wid >> 1, wc = wid & 1;
    const int nMt = (M + 127) >> 7, nNt = (N + 127) >> 7;
    const int ntiles = nMt * nNt;
    const int nk = K / BK;
    const int c = lane & 15, g = lane >> 4;
    const int dmodel = ea.H * ea.dh;

    // tile id -> (mt, nt); XCD-aware (blocks b, b+8 share an L2): the N tiles of one A row-panel stay on one XCD
    auto tile_of = [&](int id, int& mt, int& nt) {
        if ((nMt & 7) == 0) { const int xcd = id & 7, local = id >> 3; mt = (local / nNt) * 8 + xcd; nt = local % nNt; }
        else { mt = id / nNt; nt = id % nNt; }
    };
    GtState<TM> gs;
    auto setup = [&](int m0, int n0) {
        const int r = lane >> 2, sp = lane & 3;
        const int kcol = (sp ^ gl_f(r)) * EPC;
#pragma unroll
        for (int u = 0; u < 2; ++u) {     // 8 sixteen-row pieces per operand; wave takes pieces wid, wid+4
            gs.pa[u] = A + (size_t)min(m0 + 16 * (wid + 4 * u) + r, M - 1) * K + kcol;
            gs.pb[u] = Bt + (size_t)(n0 + 16 * (wid + 4 * u) + r) * ldb + kcol;
        }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ra = wr * 64 + 16 * i + c, rb = wc * 64 + 16 * i + c;
        gs.offA[i] = ra * 64 + (is_bf16_t<TM>::value ? ((g ^ gl_f(ra)) << 4) : (gl_f(ra) << 4) + g * 4);
        gs.offB[i] = 8192 + rb * 64 + (is_bf16_t<TM>::value ? ((g ^ gl_f(rb)) << 4) : (gl_f(rb) << 4) + g * 4);
    }
    auto issue = [&](char* stage) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gs.pa[u],
                                             (__attribute__((address_space(3))) void*)(stage + (wid + 4 * u) * 1024), 16, 0, 0);
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gs.pb[u],
                                             (__attribute__((address_space(3))) void*)(stage + 8192 + (wid + 4 * u) * 1024), 16, 0, 0);
            gs.pa[u] += BK; gs.pb[u] += BK;
        }
    };

    // ---- persistent loop over this workgroup's tiles.  The first two DMA stages of tile t+1 are issued BEFORE the
    // epilogue of tile t, so one workgroup's C stores overlap its own next loads (and workgroups drift out of phase).
    int tile = blockIdx.x;
    if (tile >= ntiles) return;
    int mt, nt;
    tile_of(tile, mt, nt);
    setup(mt << 7, nt << 7);
#pragma unroll
    for (int st = 0; st < GT_NSTAGE - 1; ++st)
        if (st < nk) issue(smem + st * GT_STAGE);
    bool first = true;
    while (true) {
        const int m0 = mt << 7, n0 = nt << 7;
        f32x4 acc[4][4];       // acc[j][i]: n tile j, m tile i
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int nl = n0 + wc * 64 + 4 * g;          // + 16j
        float bias[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) bias[j][e] = (ea.bias && nl + 16 * j + e < N) ? ea.bias[nl + 16 * j + e] : 0.f;

        for (int kt0 = 0; kt0 < nk; kt0 += GT_NSTAGE) {
#pragma unroll
            for (int u = 0; u < GT_NSTAGE; ++u) {
                const int kt = kt0 + u;
                if (kt < nk) {
                    // 4 DMA per wave per K tile, one later tile in flight.  At the first K tile of a later output tile the
                    // previous epilogue's loads/stores are younger than these DMAs in the in-order counter: drain everything.
                    if (kt + 1 < nk && (kt > 0 || first)) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    if (kt + GT_NSTAGE - 1 < nk) issue(smem + ((u + GT_NSTAGE - 1) % GT_NSTAGE) * GT_STAGE);
                    const char* st = smem + u * GT_STAGE;
                    if constexpr (is_bf16_t<TM>::value) {
                        bf16x8 a[4], b[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) { a[i] = *reinterpret_cast<const bf16x8*>(st + gs.offA[i]); b[i] = *reinterpret_cast<const bf16x8*>(st + gs.offB[i]); }
#pragma unroll
                        for (int j = 0; j < 4; ++j)
#pragma unroll
                            for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[j][i], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            float a[4], b[4];
#pragma unroll
                            for (int i = 0; i < 4; ++i) { a[i] = *reinterpret_cast<const float*>(st + (gs.offA[i] ^ (s << 4))); b[i] = *reinterpret_cast<const float*>(st + (gs.offB[i] ^ (s << 4))); }
#pragma unroll
                            for (int j = 0; j < 4; ++j)
#pragma unroll
                                for (int i = 0; i < 4; ++i) acc[j][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j], a[i], acc[j][i], 0, 0, 0);
                        }
                    }
                }
            }
        }
        // ---- next tile: once every wave has finished reading the ring, start its first DMA stages, then run the epilogue
        const int ntile = tile + gridDim.x;
        const bool more = ntile < ntiles;
        int mt2 = 0, nt2 = 0;
        if (more) {
            tile_of(ntile, mt2, nt2);
            __builtin_amdgcn_s_barrier();
            setup(mt2 << 7, nt2 << 7);
#pragma unroll
            for (int st = 0; st < GT_NSTAGE - 1; ++st)
                if (st < nk) issue(smem + st * GT_STAGE);
        }
        if constexpr (EK != 0) {
            // ---- fast epilogue: one base pointer per lane, rows 16 apart, column groups 16 apart
            const int mrow = m0 + wr * 64 + c;
            TC* cb = C + (size_t)mrow * N + nl;
            const TC* rb = reinterpret_cast<const TC*>(ea.resid) + (size_t)mrow * N + nl;
            const bool full = (m0 + 128 <= M) && (n0 + 128 <= N);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!full && mrow + 16 * i >= M) continue;
                float ext[4][4];
                if constexpr (EK == 2) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (full || nl + 16 * j < N) load4t(rb + (size_t)(16 * i) * N + 16 * j, ext[j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!full && nl + 16 * j >= N) continue;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[j][i][e] + bias[j][e];
                    if constexpr (EK == 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += ext[j][e];
                    }
                    store4t(cb + (size_t)(16 * i) * N + 16 * j, v);
                }
            }
        } else if (!(ea.dbg & 1)) {
            // ---- epilogue straight from the accumulators: row m = .. + 16i + c, columns nl + 16j .. +3
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = m0 + wr * 64 + 16 * i + c;
                if (m >= M) continue;
                const size_t rowoff = (size_t)m * N;
                float ext[4][4];
                const bool need_res = ea.resid != nullptr, need_aux = ea.dact != DACT_NONE;
                if (need_res || need_aux) {           // batch the residual (or act') loads of the 4 column groups
                    const TC* src = reinterpret_cast<const TC*>(need_res ? ea.resid : ea.aux);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (nl + 16 * j < N) load4t(src + rowoff + nl + 16 * j, ext[j]);
                    }
                }
                const float rsc = ea.rowscale ? ea.rowscale[m / ea.T] : 1.f;
                const uint32_t rk = ea.drop.thr ? rng_row_key(ea.drop.key, (uint32_t)m) : 0u;
                const int bsamp = (ea.mode == EPI_QKV) ? m / ea.T : 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int n = nl + 16 * j;
                    if (n >= N) continue;
                    float v[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[j][i][e] + bias[j][e] * ((ea.rowscale && ea.rowscale_bias) ? rsc : 1.f);
                    if (ea.addtab) {
                        float t4[4];
                        load4(ea.addtab + (size_t)(m % ea.tab_period) * N + n, t4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += t4[e];
                    }
                    if (ea.pre_out) store4t(reinterpret_cast<TC*>(ea.pre_out) + rowoff + n, v);
                    if (ea.act == ACT_SWISH) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = swishf_(v[e]);
                    } else if (ea.act == ACT_RELU) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    }
                    if (ea.drop.thr) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = rng_keep(rk, (uint32_t)(n + e), ea.drop.thr) ? v[e] * ea.drop.scale : 0.f;
                    }
                    if (ea.rowscale && !ea.rowscale_bias) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] *= rsc;
                    }
                    if (need_aux) {
                        float a4[4];
                        if (need_res) load4t(reinterpret_cast<const TC*>(ea.aux) + rowoff + n, a4);
                        else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) a4[e] = ext[j][e];
                        }
                        if (ea.dact == DACT_SWISH) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] *= dswishf_(a4[e]);
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = a4[e] > 0.f ? v[e] : 0.f;
                        }
                    }
                    if (need_res) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += ext[j][e];
                    }
                    if (ea.mode == EPI_STD) {
                        store4t(C + rowoff + n, v);
                    } else {      // q,k [B,H,T,dh] rows (8-byte stores); v transposed to vt [B,H,dh,T] (2-byte stores, 1/3 of one GEMM in 30)
                        int h, part, ii;
                        if (ea.head_major) { h = n / (3 * ea.dh); const int w = n - h * 3 * ea.dh; part = w / ea.dh; ii = w - part * ea.dh; }
                        else { part = n / dmodel; const int w = n - part * dmodel; h = w / ea.dh; ii = w - h * ea.dh; }
                        const int t = m - bsamp * ea.T;
                        if (part < 2) {
                            store4t(reinterpret_cast<TC*>(part == 0 ? ea.q : ea.k) + ((size_t)(bsamp * ea.H + h) * ea.T + t) * ea.dh + ii, v);
                        } else {
                            TC* dst = reinterpret_cast<TC*>(ea.vt) + ((size_t)(bsamp * ea.H + h) * ea.dh + ii) * ea.T + t;
#pragma unroll
                            for (int e = 0; e < 4; ++e) dst[(size_t)e * ea.T] = from_f<TC>(v[e]);
                        }
                    }
                }
            }
        } else if (acc[0][0][0] == 123.456f) C[0] = from_f<TC>(acc[1][3][2]);
        if (!more) break;
        tile = ntile; mt = mt2; nt = nt2; first = false;
    }
}

template <typename TM, typename TC>
static int run_nt_t(const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const EpiArgs& ea, hipStream_t s) {
    const int nMt = (M + 127) / 128, nNt = (N + 127) / 128;
    const int ntiles = nMt * nNt;
    const int grid = ntiles < 768 ? ntiles : 768;         // persistent: 3 workgroups per CU, each walks tiles `grid` apart
    const bool fast = ea.addtab == nullptr && ea.pre_out == nullptr && ea.act == ACT_NONE && ea.drop.thr == 0 && ea.rowscale == nullptr &&
                      ea.dact == DACT_NONE && ea.mode == EPI_STD && ea.dbg == 0;
    if (fast && ea.resid) hipLaunchKernelGGL((gemm_nt_t_kernel<TM, TC, 2>), dim3(grid), dim3(256), 0, s, (const TM*)A, (const TM*)Bt, (TC*)C, M, N, K, ldb, ea);
    else if (fast) hipLaunchKernelGGL((gemm_nt_t_kernel<TM, TC, 1>), dim3(grid), dim3(256), 0, s, (const TM*)A, (const TM*)Bt, (TC*)C, M, N, K, ldb, ea);
    else hipLaunchKernelGGL((gemm_nt_t_kernel<TM, TC, 0>), dim3(grid), dim3(256), 0, s, (const TM*)A, (const TM*)Bt, (TC*)C, M, N, K, ldb, ea);
    return launch_rc();
}

template <typename TA, typename TM, typename TC, int OP>
static int run_nt(const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const OpArgs& oa, const EpiArgs& ea, hipStream_t s) {
    const int nMt = (M + 127) / 128, nNt = (N + 127) / 128;
    const int a_vec_ok = (((size_t)K * sizeof(TA)) % 16 == 0) && (((uintptr_t)A) % 16 == 0);
    hipLaunchKernelGGL((gemm_nt_kernel<TA, TM, TC, OP>), dim3(nMt * nNt), dim3(256), 0, s,
                       (const TA*)A, (const TM*)Bt, (TC*)C, M, N, K, ldb, a_vec_ok, oa, ea);
    return launch_rc();
}

template <typename TA, typename TM, typename TC>
static int run_nt_op(int op, const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const OpArgs& oa, const EpiArgs& ea, hipStream_t s) {
    switch (op) {
        case OP_NONE: return run_nt<TA, TM, TC, OP_NONE>(A, Bt, C, M, N, K, ldb, oa, ea, s);
        case OP_SWISH: return run_nt<TA, TM, TC, OP_SWISH>(A, Bt, C, M, N, K, ldb, oa, ea, s);
        case OP_COLAFFINE: return run_nt<TA, TM, TC, OP_COLAFFINE>(A, Bt, C, M, N, K, ldb, oa, ea, s);
        case OP_DROPMASK: return run_nt<TA, TM, TC, OP_DROPMASK>(A, Bt, C, M, N, K, ldb, oa, ea, s);
        default: ishara_set_error("gemm_nt: unsupported operand op %d", op); return -1;
    }
}

int g_force_regstage = 0;   // NT kernel choice: 0 A-stationary kernel (gemm_as.hip) where it applies, else the 128x128 LDS-DMA tile kernel; 3 tile kernel only; 2 LDS-DMA 64x128 kernel; 1 register-staged

// The kernel a call runs on, decided here and nowhere else: launch_gemm_nt launches what this returns and gemm_nt_kernel_name names it.
// A new kernel gets an enumerator, its test here (in priority order) and a case in each of the two switches.
NtRoute gemm_nt_route(int dtA, int dtM, int dtC, int op, const void* A, int M, int N, int K, int ldb, const EpiArgs& ea) {
    const bool pro = ea.ln_gamma || ea.pa_P;             // operand prologue: only the A-stationary kernels have one
    if (dtM == DT_F16) {          // inference-only storage type: the A-stationary kernel (gemm_as_f16.hip) where it applies, else the register-staged 128x128 tile kernel
        if (op != OP_NONE) return NT_REFUSED;
        if (dtA == DT_F16 && g_force_regstage == 0 && (K == 256 || K == 512) && ldb % 64 == 0 && ((uintptr_t)A) % 16 == 0 && gemm_nt_as_applicable(dtC, M, N, K, ldb, ea)) return NT_AS_F16;
        if (pro) return NT_REFUSED;
        return (dtA == DT_F16 && (dtC == DT_F16 || dtC == DT_F32)) || (dtA == DT_F32 && dtC == DT_F16) ? NT_REG : NT_REFUSED;
    }
    if (pro && (op != OP_NONE || !gemm_nt_as_prologue_ok(dtA, dtM, dtC, M, N, K, ldb, ea))) return NT_REFUSED;
    if (g_force_regstage == 0 && gemm_nt_big_applicable(dtA, dtM, dtC, op, A, M, N, K, ldb, ea)) return NT_BIG;       // config #4's compute-heavy shapes: the 256 x 256 two-operand tile (gemm_big.hip)
    const int bk = dtM == DT_BF16 ? 32 : 16;     // K tile of the LDS-DMA kernels
    const bool dma_ok = op == OP_NONE && dtA == dtM && K % bk == 0 && ldb % (2 * bk) == 0 && ((uintptr_t)A) % 16 == 0;
    if (dma_ok && g_force_regstage == 0 && dtM == DT_BF16 && gemm_nt_cs_applicable(dtC, M, N, K, ldb, ea)) return NT_CS;                  // K = 512 / 768 -> N = 256 at training-size M: the C-stationary kernel (gemm_cs.hip)
    if (dma_ok && g_force_regstage == 0 && dtM == DT_BF16 && gemm_nt_as_applicable(dtC, M, N, K, ldb, ea)) return NT_AS;
    const bool dma_dt = (dtM == DT_F32 && dtC == DT_F32) || (dtM == DT_BF16 && (dtC == DT_BF16 || dtC == DT_F32));       // the output types the LDS-DMA tile kernels are compiled for
    if (dma_ok && dma_dt && (g_force_regstage == 0 || g_force_regstage == 3) && N % 4 == 0 && (ea.mode != EPI_QKV || ea.dh % 4 == 0)) return NT_TILE_T;
    if (dma_ok && dma_dt && g_force_regstage != 1) return NT_GLDS;
    if (dtA == dtM && dtM == dtC && (dtM == DT_F32 || dtM == DT_BF16)) return NT_REG;                                                   // f32 or bf16 throughout: every operand transform
    if (dtM == DT_BF16 && op == OP_NONE && ((dtA == DT_F32 && dtC == DT_BF16) || (dtA == DT_BF16 && dtC == DT_F32))) return NT_REG;
    return NT_REFUSED;
}

int launch_gemm_nt(int dtA, int dtM, int dtC, int op, const void* A, const void* Bt, void* C,
                   int M, int N, int K, int ldb, const OpArgs& oa, const EpiArgs& ea, hipStream_t s) {
    if (M <= 0 || N <= 0 || K <= 0) { ishara_set_error("gemm_nt: bad shape %d %d %d", M, N, K); return -1; }
    if ((dt_is16(dtA) && K % 8 != 0) || (dtA == DT_F32 && K % 4 != 0) || ((uintptr_t)A) % 16 != 0) {
        ishara_set_error("gemm_nt: A rows must be 16-byte aligned (K=%d)", K); return -1;
    }
    if (ea.mode == EPI_QKV && (ea.T % 8 != 0 || N % 8 != 0 || ea.dh % 8 != 0)) {
        ishara_set_error("gemm_nt: QKV split needs T, dh multiples of 8 (T=%d dh=%d)", ea.T, ea.dh); return -1;
    }
    const bool f16m = dtM == DT_F16;
    int rc = 1;
    switch (gemm_nt_route(dtA, dtM, dtC, op, A, M, N, K, ldb, ea)) {
        case NT_REFUSED:
            if (f16m && op != OP_NONE) ishara_set_error("gemm_nt: f16 operands take no operand transform");
            else if (f16m && (ea.ln_gamma || ea.pa_P)) ishara_set_error("gemm_nt: f16 operand prologue on a shape the A-stationary kernel does not take");
            else if (f16m) ishara_set_error("gemm_nt: unsupported f16 dtype combination %d/%d/%d", dtA, dtM, dtC);
            else if (ea.ln_gamma || ea.pa_P) ishara_set_error("gemm_nt: operand prologue requested for a shape the A-stationary kernel does not take (check gemm_nt_as_prologue_ok first)");
            else ishara_set_error("gemm_nt: unsupported dtype combination %d/%d/%d op %d", dtA, dtM, dtC, op);
            return -1;
        case NT_AS_F16: rc = launch_gemm_nt_as_f16(dtC, A, Bt, C, M, N, K, ldb, ea, s); break;
        case NT_BIG: rc = launch_gemm_nt_big(dtA, dtM, dtC, op, A, Bt, C, M, N, K, ldb, ea, s); break;
        case NT_CS: rc = launch_gemm_nt_cs(dtC, A, Bt, C, M, N, K, ldb, ea, s); break;
        case NT_AS: rc = launch_gemm_nt_as(dtC, A, Bt, C, M, N, K, ldb, ea, s); break;
        case NT_TILE_T:
            if (dtM == DT_F32) return run_nt_t<float, float>(A, Bt, C, M, N, K, ldb, ea, s);
            return dtC == DT_BF16 ? run_nt_t<bf16, bf16>(A, Bt, C, M, N, K, ldb, ea, s) : run_nt_t<bf16, float>(A, Bt, C, M, N, K, ldb, ea, s);
        case NT_GLDS:
            if (dtM == DT_F32) return run_nt_glds<float, float>(A, Bt, C, M, N, K, ldb, ea, s);
            return dtC == DT_BF16 ? run_nt_glds<bf16, bf16>(A, Bt, C, M, N, K, ldb, ea, s) : run_nt_glds<bf16, float>(A, Bt, C, M, N, K, ldb, ea, s);
        case NT_REG:
            if (f16m && dtA == DT_F32) return run_nt<float, f16, f16, OP_NONE>(A, Bt, C, M, N, K, ldb, oa, ea, s);
            if (f16m) return dtC == DT_F16 ? run_nt<f16, f16, f16, OP_NONE>(A, Bt, C, M, N, K, ldb, oa, ea, s) : run_nt<f16, f16, float, OP_NONE>(A, Bt, C, M, N, K, ldb, oa, ea, s);
            if (dtA != dtM) return run_nt<float, bf16, bf16, OP_NONE>(A, Bt, C, M, N, K, ldb, oa, ea, s);
            if (dtC != dtM) return run_nt<bf16, bf16, float, OP_NONE>(A, Bt, C, M, N, K, ldb, oa, ea, s);
            return dtM == DT_F32 ? run_nt_op<float, float, float>(op, A, Bt, C, M, N, K, ldb, oa, ea, s) : run_nt_op<bf16, bf16, bf16>(op, A, Bt, C, M, N, K, ldb, oa, ea, s);
    }
    // the A-stationary and 256 x 256 launchers answer 1 for a shape that is not theirs: gemm_nt_route has just said that it is
    if (rc == 1) { ishara_set_error("gemm_nt: internal error: the kernel gemm_nt_route chose refused the call (M=%d N=%d K=%d)", M, N, K); return -1; }
    return rc;
}

// profiler key = the prefix of the rocprof name of the kernel launch_gemm_nt launches for the same arguments
const char* gemm_nt_kernel_name(int dtA, int dtM, int dtC, int op, const void* A, int M, int N, int K, int ldb, const EpiArgs& ea) {
    const NtRoute route = gemm_nt_route(dtA, dtM, dtC, op, A, M, N, K, ldb, ea);
    // fp16 has one family label for both of its routes (NT_AS_F16, NT_REG): there is no fp16 instantiation namer
    if (dtM == DT_F16) return "gemm_nt_kernel<f16>";
    switch (route) {
        case NT_BIG: return "gemm_nt_big_kernel<bf16>";
        case NT_CS: return gemm_nt_cs_name(K, ea);
        case NT_AS: return gemm_nt_as_name(dtC, K, ea, M, N);
        case NT_TILE_T: return dtM == DT_F32 ? "gemm_nt_t_kernel<f32,f32>" : (dtC == DT_F32 ? "gemm_nt_t_kernel<bf16,f32>" : "gemm_nt_t_kernel<bf16,bf16>");
        case NT_GLDS: return dtM == DT_F32 ? "gemm_nt_glds_kernel<f32,f32>" : (dtC == DT_F32 ? "gemm_nt_glds_kernel<bf16,f32>" : "gemm_nt_glds_kernel<bf16,bf16>");
        default: break;           // NT_REG, and NT_REFUSED (nothing runs): the register-staged kernel of the types
    }
    if (dtA == DT_F32 && dtM == DT_BF16) return "gemm_nt_kernel<f32,bf16,bf16>";
    if (dtM == DT_F32) return "gemm_nt_kernel<f32,f32,f32>";
    return dtC == DT_F32 ? "gemm_nt_kernel<bf16,bf16,f32>" : "gemm_nt_kernel<bf16,bf16,bf16>";
}
