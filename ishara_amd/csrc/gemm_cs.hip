// gemm_cs.hip — "C-stationary" NT GEMM for the K = 512 -> N = 256 projections of the encoder at training-size M (gfx950), and for the
// K = 768 -> N = 256 dgrad of the QKV projection (plain epilogue only).
//
//   C[M,256] = epi( pro(A)[M,K] . Bt[256,K]^T ),  K = 64 NST in {512, 768}, bf16 operands and output, fp32 accumulate.
//
// Nothing below but the number of K chunks depends on K: the accumulator registers, the LDS ring and the wait classes of cs_stage are the same
// for NST = 8 and NST = 12 (gemm_nt_cs_kernel<0,0,12>: 79 -> 56 us per launch against the 128 x 128 tile kernel).
//
// The A-stationary kernels (gemm_as.hip) keep a wave's rows x full K in registers: at K = 512 that is 128 VGPRs, loaded in one burst that
// nothing overlaps, followed by a column loop that only writes.  At N = 256 the roles can be swapped: the fp32 accumulators of 32 rows x ALL
// 256 columns are 128 registers per wave, and both operands stream along K underneath them:
//   * A goes from global memory straight to MFMA fragment registers in chunks of 64 k (a whole 128-byte line per row and chunk), two chunks
//     in flight per wave and a third being consumed: 8 waves x 2 x 4 KB = 64 KB in flight per CU;
//   * W streams through an LDS-DMA ring of 4 stages x 32 KB (all 256 weight rows x 64 k), three stages ahead of the one being read, one
//     counted `s_waitcnt vmcnt(N)` and one barrier per stage; the bank swizzle is applied to the SOURCE address (an LDS-DMA image is
//     lane-linear): 16-byte chunk p of staged row r holds source chunk p ^ cs_swz(r);
//   * a workgroup of 8 waves owns 384 rows, one per CU (256 workgroups at M = 98304): a 256-row pass at 32 rows per wave, then a 128-row
//     pass at 16 rows per wave.  The second pass's first A chunks and weight stages are requested BEFORE the first pass's stores (loads and
//     stores retire in order on one counter: behind the stores they would wait for them).
// Same MFMA instruction, operand order (`mfma(W fragment, A fragment)`), paired weight-row permutation (a lane owns 8 consecutive columns:
// 16-byte stores), ascending order over K and epilogue arithmetic as gemm_as.hip's as_pass: the outputs are bit-identical to it.
//
// BUILD CHECK.  The A chunks and residual rows in flight are outputs of asm loads: hipcc believes them valid from the load on, so one spill
// or copy of such a register between cs_ld16 and cs_pin corrupts data silently.  The Makefile therefore compiles this file with
// -Rpass-analysis=kernel-resource-usage and fails when any kernel has scratch; re-check that, the VGPR counts (226 / 246 / 253 / 244 /
// 248 / 224 of 256 for <0,0> <1,0> <9,0> <1,2> <17,2> <0,0,12>) and the ISA between every asm load and its wait whenever ROCm is bumped.
// The library default of as_flags is stated twice: CS_DEFAULT_FLAGS below and 51 in gemm_as.hip's as_default_flags() (that file ignores bits
// 64 / 128, and both read ISHARA_AS_FLAGS): whoever changes a default bit of the A-stationary kernels changes both.
//
// hipcc's wait-counter model drains everything (`vmcnt(0)`) at the use of an ordinary load while an LDS-DMA is in flight, so every load the
// pipeline must not wait for — the A chunks and the residual rows — is an inline-asm load and every wait on the VM counter is counted by
// hand.  The K loop is fully unrolled: no back-edge at which registers could be copied while a load into them is in flight, and every count
// below is a compile-time constant.  Row blocks that are not full (the last workgroup) issue a lane-dependent number of stores, so they wait
// with vmcnt(0).
#include <cstdio>
#include <cstdlib>
#include <map>
#include "common.h"
#include "kernels.h"

enum { CS_RESID = 1, CS_DROP = 8, CS_ROWSCALE = 16 };          // the epilogue feature bits of gemm_as.hip (AS_RESID, AS_DROP, AS_ROWSCALE)
#define CS_N 256
#define CS_ROWS 384          // rows per workgroup: 256 + 128
// NST = K / 64: K chunks / weight stages per pass (64 k each): 8 (K = 512, every mask) or 12 (K = 768, the plain mask: the QKV projection's dgrad)
#define CS_RING 4
#define CS_STAGE 32768       // 256 weight rows x 128 bytes
#define CS_DPW 4             // 1 KB DMA instructions per wave and stage (32 per stage, 8 waves)
#define CS_LDS(K) (CS_RING * CS_STAGE + CS_N * 4 + 2 * (K) * 4)      // ring | bias | P, Q of the per-sample affine
// library default of as_flags as this file reads them: the A-stationary kernels' 51 | 64, the route on (14.50 -> 14.15 ms/step by same-box alternation,
// every mask of the step faster than its old kernel: DESIGN 7d); ISHARA_AS_FLAGS=51 / ishara_debug_set_as_flags(51) turn it off
#define CS_DEFAULT_FLAGS 115
#define CS_MIN_M 49153       // M > 49152: at exactly 49152 rows the A-stationary launcher still splits the columns over 2 x 256 workgroups and keeps the call

typedef __attribute__((ext_vector_type(4))) uint32_t cs_u32x4;

template <int N> DEVI void cs_wait_vm() { static_assert(N >= 0 && N < 64, "vmcnt is 6 bits"); asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// counted wait of a full row block (N0; NP with the prologue's row stores in the loop), vmcnt(0) otherwise
template <int N0, int NP> DEVI void cs_wait(bool counted, bool pout) {
    if (!counted) cs_wait_vm<0>(); else if (pout) cs_wait_vm<NP>(); else cs_wait_vm<N0>();
}
// a 16-byte global load the compiler does not know to be in flight: the caller waits (cs_wait) and then pins the use behind the wait (cs_pin)
template <int OFF> DEVI cs_u32x4 cs_ld16(const void* p) {
    cs_u32x4 r;
    asm volatile("global_load_dwordx4 %0, %1, off offset:%2" : "=v"(r) : "v"(p), "n"(OFF) : "memory");
    return r;
}
DEVI void cs_pin(cs_u32x4& r) { asm volatile("" : "+v"(r)); }
// acc = W fragment . A fragment + acc (FIRST: + 0), in place
DEVI void cs_mfma(bool first, f32x4& acc, const bf16x8& b, const cs_u32x4& a) {      // (first: a constant once the stage is unrolled)
    if (first) asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, 0" : "=&v"(acc) : "v"(b), "v"(a));
    else asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+v"(acc) : "v"(b), "v"(a));
}
// swizzle of a staged weight row (128 bytes = 8 chunks of 16): chunk q of row r sits at position q ^ cs_swz(r).  Row bits 1 and 4, not bit 0:
// a ds_read_b128 is served in groups of 16 lanes = two k groups g x 8 fragment rows 8*(c>>2) + (c&3); rows of equal parity (c bit 0: the two
// 128-byte halves of the 256-byte bank row) must take 8 distinct positions — bit 0 of the position separates the two k groups, bits 1 and 2
// the four rows (c bit 1 = row bit 1, c bit 3 = row bit 4).
DEVI int cs_swz(int r) { return (r & 2) | (((r >> 4) & 1) << 2); }
DEVI void cs_unpack(const cs_u32x4& r, float (&v)[8]) {
#pragma unroll
    for (int h = 0; h < 4; ++h) { v[2 * h] = __uint_as_float(r[h] << 16); v[2 * h + 1] = __uint_as_float(r[h] & 0xffff0000u); }
}
DEVI void cs_st_pk(bf16* p, const bf16x8& t, bool nt) {
    if (nt) __builtin_nontemporal_store(t, reinterpret_cast<bf16x8*>(p)); else *reinterpret_cast<bf16x8*>(p) = t;
}

// what a lane needs all kernel long
struct CsLane {
    const bf16* bsrc[CS_DPW];     // this lane's source of the wave's DMA pieces of stage 0
    int off0, off1;               // fragment-read offsets inside a stage: even / odd 32-k step of the chunk, tile pair 0, tile 0
    int wid, c, g;
};
// rows of one pass: RT row tiles of 16 per wave
template <int RT> struct CsRows {
    const bf16* ap[RT];           // A + row * K + 8 g
    int mrow[RT];                 // clamped row
    cs_u32x4 a[3][RT][2];         // three K chunks: two in flight, one consumed
};
template <int RT, int K> DEVI void cs_rows_init(CsRows<RT>& r, const bf16* __restrict__ A, int M, int mw, const CsLane& L) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        r.mrow[i] = min(mw + 16 * i + L.c, M - 1);
        r.ap[i] = A + (size_t)r.mrow[i] * K + L.g * 8;
    }
}
// A chunk S -> buffer S % 3: lane (c, g) of row tile i takes row 16i + c, k = 64 S + 32 kt + 8 g .. +7
template <int RT, int S> DEVI void cs_load_a(CsRows<RT>& r) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        r.a[S % 3][i][0] = cs_ld16<S * 128>(r.ap[i]);
        r.a[S % 3][i][1] = cs_ld16<S * 128 + 64>(r.ap[i]);
    }
}
// weight stage S -> ring slot S % 4
template <int S> DEVI void cs_issue_w(const CsLane& L, char* smem) {
#pragma unroll
    for (int t = 0; t < CS_DPW; ++t) {
        const bf16* src = L.bsrc[t];
        asm volatile("" : "+v"(src));          // (formed again at every issue: hipcc otherwise keeps all 32 stage addresses of the first pass alive for the second)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + S * 64),
                                         (__attribute__((address_space(3))) void*)(smem + (S % CS_RING) * CS_STAGE + (L.wid * CS_DPW + t) * 1024), 16, 0, 0);
    }
}
// what a pass expects to be under way when it starts: A chunks 0, 1 and weight stages 0, 1, 2 (in this order)
template <int RT> DEVI void cs_prefetch(CsRows<RT>& r, const CsLane& L, char* smem) {
    cs_load_a<RT, 0>(r);
    cs_load_a<RT, 1>(r);
    cs_issue_w<0>(L, smem);
    cs_issue_w<1>(L, smem);
    cs_issue_w<2>(L, smem);
}
#define CS_PREFETCH_OPS(RT) (2 * 2 * (RT) + 3 * CS_DPW)

// K chunk / weight stage S of a pass of NST stages.  VM operations of a wave, in issue order (NA = 2 RT loads per A chunk, D = 4 DMAs per
// stage, P = NA stores of the prologue's rows when they are written, E = stores of the previous pass's epilogue), at NST = 8:
//     A0 A1 D0 D1 D2 [E] | A2 D3 P0 | A3 D4 P1 | A4 D5 P2 | A5 D6 P3 | A6 D7 P4 | A7 P5 | P6 | P7
// and at NST = 12 four more middle stages `A(S+2) D(S+3) P(S)`.  Stage S needs A(S) and D(S): everything younger than the later of the two
// may stay in flight.  From S = 2 on the later one is A(S), issued by stage S - 2 in front of D(S+1) P(S-2) | A(S+1) D(S+2) P(S-1), of which
// D(S+2) is missing at S = NST - 2 and all but the stores at S = NST - 1: the five classes below do not depend on NST otherwise.
template <int MASK, int PRO, int NST, int RT, int E, int S>
DEVI void cs_stage(CsRows<RT>& r, const CsLane& L, char* smem, const float* pq_s, f32x4 (&acc)[8][2][RT], bf16* pro_out, int M, int mw,
                   bool full, bool pout, bool nt_side) {
    constexpr int NA = 2 * RT, D = CS_DPW, K = 64 * NST;
    static_assert(NST >= 5 && S < NST, "the wait classes below need a middle stage");
    if constexpr (S == 0) cs_wait<2 * D + E, 2 * D + E>(full, pout);
    else if constexpr (S == 1) cs_wait<2 * D + E + NA, 2 * D + E + NA + NA>(full, pout);
    else if constexpr (S <= NST - 3) cs_wait<2 * D + NA, 2 * D + NA + 2 * NA>(full, pout);
    else if constexpr (S == NST - 2) cs_wait<D + NA, D + NA + 2 * NA>(full, pout);
    else cs_wait<0, 2 * NA>(full, pout);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // stage S has landed for every wave; every wave is done reading stage S - 1
    if constexpr (S + 2 < NST) cs_load_a<RT, S + 2>(r);
    if constexpr (S + 3 < NST) cs_issue_w<S + 3>(L, smem);        // into the slot of stage S - 1
    constexpr int B = S % 3;
#pragma unroll
    for (int i = 0; i < RT; ++i) { cs_pin(r.a[B][i][0]); cs_pin(r.a[B][i][1]); }
    if constexpr (PRO == 2) {              // per-sample affine on the chunk as it arrives: a' = bf16(a * P + Q), as as_pass rounds it
#pragma unroll
        for (int kt = 0; kt < 2; ++kt) {
            const float* cp = pq_s + 64 * S + 32 * kt + 8 * L.g;
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(cp), w1 = *reinterpret_cast<const f32x4*>(cp + 4);
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(cp + K), b1 = *reinterpret_cast<const f32x4*>(cp + K + 4);
            float wv[8], bv[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { wv[e] = w0[e]; wv[4 + e] = w1[e]; bv[e] = b0[e]; bv[4 + e] = b1[e]; }
#pragma unroll
            for (int i = 0; i < RT; ++i) {
                float v[8];
                cs_unpack(r.a[B][i][kt], v);
                bf16x8 t;
#pragma unroll
                for (int e = 0; e < 8; ++e) t[e] = (bf16)(v[e] * wv[e] + bv[e]);
                r.a[B][i][kt] = __builtin_bit_cast(cs_u32x4, t);
                if (pout && (full || mw + 16 * i + L.c < M))
                    cs_st_pk(pro_out + (size_t)r.mrow[i] * K + L.g * 8 + 64 * S + 32 * kt, t, nt_side);
            }
        }
    }
    // acc[p][jj][i] += W[32 p + 8 (t >> 2) + 4 jj + (t & 3), k] * A[16 i + c, k]  (t: the MFMA tile row)
    // The MFMAs are inline asm with the accumulator tied to itself and run in the order written; the fragment reads run two tile pairs ahead
    // of them, by hand.  (As builtins, hipcc renames the 128 accumulator registers at every stage of the unrolled loop, hoists a whole
    // stage of fragment reads and spills — also A chunk registers whose loads are in flight.)
    const char* st = smem + (S % CS_RING) * CS_STAGE;
    auto frag = [&](int q, int jj) { return *reinterpret_cast<const bf16x8*>(st + ((q >> 3) ? L.off1 : L.off0) + (32 * (q & 7) + 4 * jj) * 128); };
    bf16x8 b0 = frag(0, 0), b1 = frag(0, 1), c0 = frag(1, 0), c1 = frag(1, 1);
    if constexpr (PRO != 0) asm volatile("s_nop 1");          // a chunk the VALU has just written -> MFMA operand
#pragma unroll
    for (int q = 0; q < 16; ++q) {         // q = 8 kt + p; the reads of pair q + 2 are issued before the MFMAs of pair q
        const int kt = q >> 3, p = q & 7;
        bf16x8 n0 = c0, n1 = c1;
        if (q + 2 < 16) { n0 = frag(q + 2, 0); n1 = frag(q + 2, 1); }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            cs_mfma(S == 0 && q < 8, acc[p][0][i], b0, r.a[B][i][kt]);
            cs_mfma(S == 0 && q < 8, acc[p][1][i], b1, r.a[B][i][kt]);
        }
        b0 = c0; b1 = c1; c0 = n0; c1 = n1;
    }
}

// stages S .. NST - 1 of a pass, in order (the K loop, fully unrolled)
template <int MASK, int PRO, int NST, int RT, int E, int S>
DEVI void cs_stages(CsRows<RT>& r, const CsLane& L, char* smem, const float* pq_s, f32x4 (&acc)[8][2][RT], bf16* pro_out, int M, int mw,
                    bool full, bool pout, bool nt_side) {
    cs_stage<MASK, PRO, NST, RT, E, S>(r, L, smem, pq_s, acc, pro_out, M, mw, full, pout, nt_side);
    if constexpr (S + 1 < NST) cs_stages<MASK, PRO, NST, RT, E, S + 1>(r, L, smem, pq_s, acc, pro_out, M, mw, full, pout, nt_side);
}

// One pass over the rows [m_base, m_base + 128 RT) (wave w: 16 RT rows from m_base + 16 RT w); started with cs_prefetch under way and E
// stores of the previous pass younger than it.  `hand` requests the next pass's prefetch; it runs after the K loop (the ring is free) and
// before this pass's stores.  HOPS: the VM operations it issues (0: last pass).
template <int MASK, int PRO, int NST, int RT, int E, typename HAND>
DEVI void cs_pass(CsRows<RT>& r, const CsLane& L, bf16* __restrict__ C, int M, const EpiArgs& ea, char* smem, const float* bias_s, const float* pq_s,
                  int m_base, float rsc, int hops, HAND hand) {
    const int mw = m_base + L.wid * 16 * RT;
    const bool full = m_base + 128 * RT <= M;
    const bool pout = PRO != 0 && ea.pro_out != nullptr;
    const bool nt_side = (ea.as_flags & 2) != 0;
    constexpr bool f_resid = (MASK & CS_RESID) != 0, f_drop = (MASK & CS_DROP) != 0, f_rowscale = (MASK & CS_ROWSCALE) != 0;
    f32x4 acc[8][2][RT];          // (first written by stage 0's MFMAs: acc = 0 + W . A)
    bf16* po = reinterpret_cast<bf16*>(ea.pro_out);
    cs_stages<MASK, PRO, NST, RT, E, 0>(r, L, smem, pq_s, acc, po, M, mw, full, pout, nt_side);

    asm volatile("s_nop 15");          // the last MFMAs' results -> the compiler's epilogue code
    // residual rows first (the A chunk registers are free), then the next pass's prefetch, then the stores
    size_t eoff[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) eoff[i] = (size_t)r.mrow[i] * CS_N + 8 * L.g;
    cs_u32x4 rs[RT][8];
    if constexpr (f_resid) {
        const bf16* resid = reinterpret_cast<const bf16*>(ea.resid);
#pragma unroll
        for (int i = 0; i < RT; ++i) {
            const bf16* rp = resid + eoff[i];
            rs[i][0] = cs_ld16<0>(rp);   rs[i][1] = cs_ld16<64>(rp);  rs[i][2] = cs_ld16<128>(rp); rs[i][3] = cs_ld16<192>(rp);
            rs[i][4] = cs_ld16<256>(rp); rs[i][5] = cs_ld16<320>(rp); rs[i][6] = cs_ld16<384>(rp); rs[i][7] = cs_ld16<448>(rp);
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();          // every wave is done reading the ring before the next pass refills it
    hand();
    if constexpr (f_resid) {
        if (hops) cs_wait_vm<CS_PREFETCH_OPS(1)>(); else cs_wait_vm<0>();      // (the next pass is the 16-rows-per-wave one)
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int p = 0; p < 8; ++p) cs_pin(rs[i][p]);
    }
    uint32_t rk[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) rk[i] = f_drop ? rng_row_key(ea.drop.key, (uint32_t)(mw + 16 * i + L.c)) : 0u;
    // epilogue from the accumulators, arithmetic in as_pass's order: lane owns row 16 i + c and, per tile pair p, columns 32 p + 8 g .. +7.
    // The two pairs 2 q, 2 q + 1 of a row are stored back to back: the two 64-byte halves of a 128-byte line.
#pragma unroll
    for (int i = 0; i < RT; ++i) {
        const int m = mw + 16 * i + L.c;
        if (!full && m >= M) continue;
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int n = 32 * p + 8 * L.g;
            float bias[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_s + n + 4 * h);
#pragma unroll
                for (int e = 0; e < 4; ++e) bias[4 * h + e] = bv[e];
            }
            float v[8];
            const float bsc = (f_rowscale && ea.rowscale_bias) ? rsc : 1.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = acc[p][0][i][e] + bias[e] * bsc; v[4 + e] = acc[p][1][i][e] + bias[4 + e] * bsc; }
            if constexpr (f_drop) rng_apply<8>(rk[i], (uint32_t)n, ea.drop.thr, ea.drop.scale, v);
            if (f_rowscale && !ea.rowscale_bias) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] *= rsc;
            }
            if constexpr (f_resid) {
                float x[8];
                cs_unpack(rs[i][p], x);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += x[e];
            }
            store8(C + eoff[i] + 32 * p, v);
        }
    }
}

template <int MASK, int PRO, int NST>
DEVI void cs_body(const bf16* __restrict__ A, const bf16* __restrict__ Bt, bf16* __restrict__ C, int M, int ldb, const EpiArgs& ea) {
    constexpr int K = 64 * NST;
    extern __shared__ __attribute__((aligned(16))) char cs_smem[];
    float* bias_s = reinterpret_cast<float*>(cs_smem + CS_RING * CS_STAGE);
    float* pq_s = bias_s + CS_N;
    const int tid = threadIdx.x, lane = tid & 63;
    const int m_base = blockIdx.x * CS_ROWS;
    const int bsm = min(m_base, M - 1) / max(ea.T, 1);          // PRO 2 / row scale: the workgroup's rows lie in ONE sample (launcher)
    for (int n = tid; n < CS_N; n += 512) bias_s[n] = ea.bias ? ea.bias[n] : 0.f;
    if constexpr (PRO == 2) {
        const float* c0 = ea.pa_P + (size_t)bsm * K;
        const float* c1 = ea.pa_Q + (size_t)bsm * K;
        for (int x = tid; x < K; x += 512) { pq_s[x] = c0[x]; pq_s[K + x] = c1[x]; }
    }
    float rsc = 1.f;
    if constexpr ((MASK & CS_ROWSCALE) != 0) rsc = ea.rowscale[bsm];
    __syncthreads();          // (ordinary loads end here: from the first DMA on, every VM wait is counted by hand)
    asm volatile("" : "+v"(rsc));

    CsLane L;
    L.wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    L.c = lane & 15; L.g = lane >> 4;
#pragma unroll
    for (int t = 0; t < CS_DPW; ++t) {      // DMA instruction u = 4 wid + t moves bytes [1024 u, +1024) of a stage: rows 8 u .. 8 u + 7
        const int rr = (L.wid * CS_DPW + t) * 8 + (lane >> 3), p = lane & 7;
        L.bsrc[t] = Bt + (size_t)rr * ldb + ((p ^ cs_swz(rr)) << 3);
    }
    const int frow = 8 * (L.c >> 2) + (L.c & 3);
    const int sx = L.g ^ cs_swz(frow);
    L.off0 = frow * 128 + (sx << 4);
    L.off1 = frow * 128 + ((sx ^ 4) << 4);

    const bool two = m_base + 256 < M;
    CsRows<2> r1;
    CsRows<1> r2;
    cs_rows_init<2, K>(r1, A, M, m_base + L.wid * 32, L);
    cs_prefetch<2>(r1, L, cs_smem);
    cs_pass<MASK, PRO, NST, 2, 0>(r1, L, C, M, ea, cs_smem, bias_s, pq_s, m_base, rsc, two ? CS_PREFETCH_OPS(1) : 0, [&]() {
        if (two) {
            cs_rows_init<1, K>(r2, A, M, m_base + 256 + L.wid * 16, L);
            cs_prefetch<1>(r2, L, cs_smem);
        }
    });
    // the first pass was full when there is a second one: E = its 2 x 8 stores per lane
    if (two) cs_pass<MASK, PRO, NST, 1, 16>(r2, L, C, M, ea, cs_smem, bias_s, pq_s, m_base + 256, rsc, 0, []() {});
}
// Two overloads, not one template with a defaulted NST: the K = 512 kernels keep their two-argument rocprof names gemm_nt_cs_kernel<MASK, PRO>,
// the K = 768 one is gemm_nt_cs_kernel<0, 0, 12>.
template <int MASK, int PRO>
__global__ __launch_bounds__(512, 1) void gemm_nt_cs_kernel(const bf16* __restrict__ A, const bf16* __restrict__ Bt, bf16* __restrict__ C, int M, int ldb, EpiArgs ea) {
    cs_body<MASK, PRO, 8>(A, Bt, C, M, ldb, ea);
}
template <int MASK, int PRO, int NST>
__global__ __launch_bounds__(512, 1) void gemm_nt_cs_kernel(const bf16* __restrict__ A, const bf16* __restrict__ Bt, bf16* __restrict__ C, int M, int ldb, EpiArgs ea) {
    static_assert(NST != 8, "K = 512 is the two-argument overload");
    cs_body<MASK, PRO, NST>(A, Bt, C, M, ldb, ea);
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------
static int cs_mask_of(const EpiArgs& ea) {      // as gemm_as.hip's as_mask_of
    return (ea.resid ? 1 : 0) | (ea.dact != DACT_NONE ? 2 : 0) | (ea.act != ACT_NONE ? 4 : 0) | (ea.drop.thr ? 8 : 0) | (ea.rowscale ? 16 : 0) |
           (ea.pre_out ? 32 : 0) | (ea.mode == EPI_QKV ? 64 : 0) | (ea.addtab ? 128 : 0);
}
// as_flags as this route reads them: the per-call value, else ishara_debug_set_as_flags, else ISHARA_AS_FLAGS, else the library default
// CS_DEFAULT_FLAGS.  115 = 51 (the A-stationary kernels' switches, gemm_as.hip) | 64 (this route on); 128: ignore the row threshold (tests);
// 256: K = 768 stays on the 128 x 128 tile kernel (A/B runs of the QKV projection's dgrad inside one build)
static int cs_flags(const EpiArgs& ea) {
    static const int v = getenv("ISHARA_AS_FLAGS") ? atoi(getenv("ISHARA_AS_FLAGS")) : CS_DEFAULT_FLAGS;
    return ea.as_flags >= 0 ? ea.as_flags : (g_as_flags_override >= 0 ? g_as_flags_override : v);
}
bool gemm_nt_cs_applicable(int dtC, int M, int N, int K, int ldb, const EpiArgs& ea) {
    if (dtC != DT_BF16 || (K != 512 && K != 768) || N != CS_N || M < 1 || ldb < K || ldb % 8 != 0) return false;
    const int flags = cs_flags(ea);
    if (!(flags & 64)) return false;
    if (K == 768 && ((flags & 256) || ea.pa_P || cs_mask_of(ea) != 0)) return false;          // K = 768: the plain mask alone (<0,0,12>)
    if (ea.n_valid || ea.dbg || (ea.ldc && ea.ldc != CS_N) || ea.ln_gamma) return false;
    if (!(flags & 128) && M < CS_MIN_M) return false;
    const int mask = cs_mask_of(ea);
    if (ea.pa_P) return ea.pa_Q && ea.T > 0 && ea.T % CS_ROWS == 0 && (mask == CS_RESID || mask == (CS_RESID | CS_ROWSCALE));
    return mask == 0 || mask == CS_RESID || mask == (CS_RESID | CS_DROP);
}
const char* gemm_nt_cs_name(int K, const EpiArgs& ea) {
    static std::map<int, std::string> names;
    const int mask = cs_mask_of(ea), pro = ea.pa_P ? 2 : 0, key = mask | pro << 8 | (K == 768) << 12;
    auto it = names.find(key);
    if (it == names.end()) {
        char buf[64];
        if (K == 768) snprintf(buf, sizeof buf, "gemm_nt_cs_kernel<%d,%d,12>", mask, pro);
        else snprintf(buf, sizeof buf, "gemm_nt_cs_kernel<%d,%d>", mask, pro);
        it = names.emplace(key, buf).first;
    }
    return it->second.c_str();
}
typedef void (*cs_kernel_t)(const bf16*, const bf16*, bf16*, int, int, EpiArgs);
template <int MASK, int PRO, int NST = 8>
static int cs_launch(const void* A, const void* Bt, void* C, int M, int ldb, const EpiArgs& ea, hipStream_t s) {
    cs_kernel_t kern;
    if constexpr (NST == 8) kern = gemm_nt_cs_kernel<MASK, PRO>; else kern = gemm_nt_cs_kernel<MASK, PRO, NST>;
    constexpr int lds = CS_LDS(64 * NST);
    static int ready = 0;          // dynamic LDS above 64 KB needs the attribute once per kernel
    if (!ready) ready = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds) == hipSuccess ? 1 : -1;
    if (ready < 0) { ishara_set_error("gemm_nt_cs: %d bytes of LDS refused", lds); return -1; }
    hipLaunchKernelGGL(kern, dim3((M + CS_ROWS - 1) / CS_ROWS), dim3(512), lds, s, (const bf16*)A, (const bf16*)Bt, (bf16*)C, M, ldb, ea);
    return launch_rc();
}
// returns 1 when the call is not one this kernel takes
int launch_gemm_nt_cs(int dtC, const void* A, const void* Bt, void* C, int M, int N, int K, int ldb, const EpiArgs& ea_in, hipStream_t s) {
    if (!gemm_nt_cs_applicable(dtC, M, N, K, ldb, ea_in)) return 1;
    EpiArgs ea = ea_in;
    ea.as_flags = cs_flags(ea_in);
    const int mask = cs_mask_of(ea);
    if (K == 768) return cs_launch<0, 0, 12>(A, Bt, C, M, ldb, ea, s);
    if (ea.pa_P) return mask == CS_RESID ? cs_launch<CS_RESID, 2>(A, Bt, C, M, ldb, ea, s) : cs_launch<CS_RESID | CS_ROWSCALE, 2>(A, Bt, C, M, ldb, ea, s);
    if (mask == 0) return cs_launch<0, 0>(A, Bt, C, M, ldb, ea, s);
    if (mask == CS_RESID) return cs_launch<CS_RESID, 0>(A, Bt, C, M, ldb, ea, s);
    return cs_launch<CS_RESID | CS_DROP, 0>(A, Bt, C, M, ldb, ea, s);
}
