// CTC forced alignment: the best single path of a known label through the CTC lattice (Viterbi), one frame span and one confidence per
// symbol.  The semantics are stated in ishara_amd/ctc_align.py (module docstring) and implemented exactly here: the path maximises the sum
// of the RAW logits along it, carried in fp64 with one add per frame in frame order, ties broken stay > s-1 > s-2, so that every integer
// output equals the host reference's on every input.
//
// One 256-thread workgroup per sample, three phases:
//   1  wave 0         the max-plus recursion in the arrangement of ctc_kernel (ctc.hip): state s = lane + 64 k in registers, the s-1 / s-2
//                     neighbours by two wave rotations (DPP) per frame with the k-1 carry at lanes 0 and 1, the emissions gathered a group of 8
//                     frames ahead, a compile-time register count NK for short labels.  The chain is fp64 compare / select / add: no exp,
//                     no log, no barrier.  Each lane packs the 2-bit back-pointers of its (up to 8) states of a frame into one 16-bit word:
//                     a frame is 64 words = 128 bytes, kept in LDS where T * 128 bytes fit (BPLDS), in the caller's workspace otherwise.
//                     Then the backtrace, by the same wave: the state is wave-uniform, every lane re-reads the words IT wrote (a group of
//                     frames ahead of the chain) and the chain picks the word of lane s % 64 by a lane read -- no memory access on it.
//      waves 1-3      meanwhile: per frame the row maximum m_t and sum_c expf(x_c - m_t) (LDS), and the fp64 sums of m_t and of logf(sum)
//   2  all threads    per frame: span edges (start where the symbol changes, end likewise) and the softmax value of the emitted symbol
//   3  all threads    per symbol: the mean of those values over its span, in frame order (fp64 accumulator); thread 0: the score
// Nothing is accumulated by atomics and every reduction has a fixed order: the outputs are bit-identical from run to run.
//
// Indices derived from data: the back-pointer is two bits, the state only ever decreases from S-1 and is clamped at 0, so frame_pos stays
// in [-1, len); span bounds read back from memory are clamped to [0, T] before they index anything -- whatever the logits hold.
#include <type_traits>
#include "ctc_lattice.h"                                // ctc_ns: the registers per lane of the lattice

#define ALIGN_DEAD (-__builtin_huge_val())
// LDS of one workgroup: (m_t, sum_t) [T] and ext [64 NS] always, the back-pointer rows [T][64] u16 on the fast path; the static part (label
// length, reduction slots, the block-wide votes: 336 bytes) is below ALIGN_LDS_STATIC.  Above the 64 KiB every launch is granted the
// kernel's limit is raised, up to the CU's 160 KiB.
static constexpr size_t ALIGN_LDS_STATIC = 512, ALIGN_LDS_DEFAULT = 65536, ALIGN_LDS_MAX = 163840;
static size_t align_lds_bytes(int T, int L, bool bp) { return (size_t)T * 8 + (size_t)256 * ctc_ns(L) + (bp ? (size_t)T * 128 : 0); }
bool ctc_align_bp_in_lds(int T, int L) { return align_lds_bytes(T, L, true) + ALIGN_LDS_STATIC <= ALIGN_LDS_MAX; }
size_t ctc_align_workspace_bytes(int B, int T, int L) { return B == 0 ? 0 : (ctc_align_bp_in_lds(T, L) ? 128 : (size_t)B * T * 128); }

// lane l takes the value of lane l - 1, lane 0 that of lane 63: the whole-wave rotation of the DPP data path (the wave is fully active where
// this is called).  In registers, where __shfl goes through the LDS crossbar and costs its latency on the recursion's chain twice a frame.
DEVI double wave_ror1(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x13C, 0xF, 0xF, false);      // 0x13C: wave_ror:1
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x13C, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

// VL (ishara_ctc_align_ex): the sample has Tn = frame_len[b] frames of the buffer's Ts; Ts stays the stride of the logits, of frame_pos, of
// the back-pointer workspace and of the LDS layout, Tn takes every other role and frame_pos[b, t >= Tn] = -1.  A frame_len[b] outside
// [1, Ts] is a sample without an alignment.
template <int NS, bool BPLDS, bool VL>
__global__ __launch_bounds__(256) void ctc_align_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int Ts, int C, int L,
                                                        int blank, uint16_t* __restrict__ ws, int* __restrict__ frame_pos, int* __restrict__ start,
                                                        int* __restrict__ end, float* __restrict__ conf, float* __restrict__ score,
                                                        const int* __restrict__ frame_len) {
    constexpr int SP = 64 * NS;
    extern __shared__ float2 sh_ms[];
    float2* ms = sh_ms;                                          // [Ts] (m_t, sum_c expf(x_c - m_t)); phase 2 puts the emitted symbol's softmax in .x
    int* ext = reinterpret_cast<int*>(ms + Ts);                  // [SP]
    uint16_t* bp = BPLDS ? reinterpret_cast<uint16_t*>(ext + SP) : ws + (size_t)blockIdx.x * Ts * 64;      // [Ts][64]
    __shared__ int s_len;
    __shared__ double s_red[2][4], s_v;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int Tn = Ts;
    if (VL && frame_len) { Tn = frame_len[b]; if (Tn < 1 || Tn > Ts) Tn = 0; }
    const float* lg = logits + (size_t)b * Ts * C;
    const int64_t* lab = labels + (size_t)b * L;
    int* fpos = frame_pos + (size_t)b * Ts;
    int* st = start + (size_t)b * L;
    int* en = end + (size_t)b * L;
    float* cf = conf + (size_t)b * L;

    // len = entries before the first blank (L <= 255: one thread per entry); repeats and out-of-range values among them
    const int64_t mine = tid < L ? lab[tid] : (int64_t)blank;
    if (tid == 0) s_len = L;
    __syncthreads();
    if (tid < L && mine == blank) atomicMin(&s_len, tid);
    __syncthreads();
    const int len = s_len, S = 2 * len + 1;
    const int rep = __syncthreads_count(tid >= 1 && tid < len && mine == lab[tid >= 1 ? tid - 1 : 0]);
    const int bad = __syncthreads_or(tid < len && (mine < 0 || mine >= C));
    if (tid < L) { st[tid] = -1; en[tid] = -1; }
    if (bad || Tn < len + rep || (VL && Tn == 0)) {              // no alignment (workgroup-uniform): the contract's constants
        for (int t = tid; t < Ts; t += 256) fpos[t] = -1;
        if (tid < L) cf[tid] = 0.f;
        if (tid == 0) score[b] = -1e30f;
        return;
    }
    if (VL)
        for (int t = Tn + tid; t < Ts; t += 256) fpos[t] = -1;
    for (int s = tid; s < SP; s += 256) {
        const int64_t v = ((s & 1) && (s >> 1) < len) ? lab[s >> 1] : (int64_t)blank;
        ext[s] = (v < 0 || v >= C) ? blank : (int)v;
    }
    __syncthreads();

    auto recursion = [&](auto nkc) {
        constexpr int NK = decltype(nkc)::value;
        constexpr int KM = NK ? NK : NS;
        const int nk = NK ? NK : ((S + 63) >> 6);
        bool act[NS], skp[NS];
        int my[NS];
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int s = lane + 64 * k;
            my[k] = ext[s];
            act[k] = s < S;
            skp[k] = act[k] && s >= 2 && my[k] != blank && my[k] != ext[s >= 2 ? s - 2 : 0];      // s-2 -> s
        }
        float em[8][NS], emn[8][NS];
        auto gather = [&](int t0, float (&dst)[8][NS]) {         // raw logits of frames t0 .. t0 + 7 (loads only)
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = min(t0 + u, Tn - 1);
#pragma unroll
                for (int k = 0; k < KM; ++k)
                    if (NK != 0 || k < nk) dst[u][k] = lg[(size_t)t * C + my[k]];
            }
        };
        double v[NS];
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int s = lane + 64 * k;
            v[k] = (act[k] && (s == 0 || (s == 1 && len > 0))) ? (double)lg[my[k]] : ALIGN_DEAD;
        }
        gather(1, em);
        for (int t0 = 1; t0 < Tn; t0 += 8) {
            if (t0 + 8 < Tn) gather(t0 + 8, emn);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = t0 + u;
                if (t < Tn) {
                    double r1[NS], r2[NS], n[NS];
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (NK != 0 || k < nk) { r1[k] = wave_ror1(v[k]); r2[k] = wave_ror1(r1[k]); }
                    uint32_t word = 0;
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (NK != 0 || k < nk) {
                            // lanes 0 (and 1) take the neighbours from lanes 63 (and 62) of the previous k
                            const double a1 = lane >= 1 ? r1[k] : (k >= 1 ? r1[k >= 1 ? k - 1 : 0] : ALIGN_DEAD);
                            const double a2 = lane >= 2 ? r2[k] : (k >= 1 ? r2[k >= 1 ? k - 1 : 0] : ALIGN_DEAD);
                            const double p2 = skp[k] ? a2 : ALIGN_DEAD;
                            double best = v[k];                  // strictly greater replaces: stay, then s-1, then s-2
                            uint32_t back = 0;
                            if (a1 > best) { best = a1; back = 1; }
                            if (p2 > best) { best = p2; back = 2; }
                            n[k] = act[k] ? best + (double)em[u][k] : ALIGN_DEAD;
                            word |= back << (2 * k);
                        }
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (NK != 0 || k < nk) v[k] = n[k];
                    bp[(size_t)t * 64 + lane] = (uint16_t)word;
                }
            }
            if (t0 + 8 < Tn) {
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (NK != 0 || k < nk) em[u][k] = emn[u][k];
            }
        }
        // the end: S-1, unless v[S-2] is strictly greater (and there is a label)
        double c1 = ALIGN_DEAD, c2 = ALIGN_DEAD;
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int s = lane + 64 * k;
            if (s == S - 1) c1 = v[k];
            if (s == S - 2) c2 = v[k];
        }
        const double v1 = __shfl(c1, (S - 1) & 63, 64), v2 = __shfl(c2, (S + 62) & 63, 64);
        const bool second = len > 0 && v2 > v1;
        if (lane == 0) s_v = second ? v2 : v1;
        int s = __builtin_amdgcn_readfirstlane(second ? S - 2 : S - 1);
        // backtrace: frames tb, tb - 1, .., tb - 7 per group; every lane holds its own words of the group, the next group's already in flight
        uint32_t w[8], wn[8];
        auto fetch = [&](int tb, uint32_t (&dst)[8]) {
#pragma unroll
            for (int u = 0; u < 8; ++u) dst[u] = bp[(size_t)max(tb - u, 1) * 64 + lane];
        };
        if (Tn > 1) fetch(Tn - 1, w);
        for (int tb = Tn - 1; tb >= 0; tb -= 8) {
            if (tb - 8 >= 1) fetch(tb - 8, wn);
            int out = -1;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = tb - u;
                if (t >= 0) {
                    if (lane == u) out = (s & 1) ? (s >> 1) : -1;
                    if (t > 0) {
                        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)w[u], s & 63);
                        s = max(s - (int)((word >> (2 * (s >> 6))) & 3u), 0);
                    }
                }
            }
            if (lane < 8 && tb - lane >= 0) fpos[tb - lane] = out;
            if (tb - 8 >= 1) {
#pragma unroll
                for (int u = 0; u < 8; ++u) w[u] = wn[u];
            }
        }
    };
    if (wave == 0) {
        const int nkb = (S + 63) >> 6;
        if (NS >= 2 && nkb == 1) recursion(std::integral_constant<int, 1>{});
        else if (NS >= 3 && nkb == 2) recursion(std::integral_constant<int, 2>{});
        else recursion(std::integral_constant<int, 0>{});
    } else {
        double sm = 0.0, sl = 0.0;
        for (int t = tid - 64; t < Tn; t += 192) {
            float m = lg[(size_t)t * C];
            for (int c = 1; c < C; ++c) m = fmaxf(m, lg[(size_t)t * C + c]);
            float a = 0.f;
            for (int c = 0; c < C; ++c) a += expf(lg[(size_t)t * C + c] - m);
            ms[t] = make_float2(m, a);
            sm += (double)m;
            sl += (double)logf(a);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sm += __shfl_xor(sm, o, 64); sl += __shfl_xor(sl, o, 64); }
        if (lane == 0) { s_red[0][wave] = sm; s_red[1][wave] = sl; }
    }
    __threadfence_block();
    __syncthreads();
    if (tid == 0) score[b] = (float)((s_v - ((s_red[0][1] + s_red[0][2]) + s_red[0][3])) - ((s_red[1][1] + s_red[1][2]) + s_red[1][3]));
    // ---- phase 2: per frame, the span edges and the softmax value of the emitted symbol
    for (int t = tid; t < Tn; t += 256) {
        const int i = min(fpos[t], len - 1);
        if (i >= 0) {
            if (t == 0 || fpos[t - 1] != i) st[i] = t;
            if (t == Tn - 1 || fpos[t + 1] != i) en[i] = t + 1;
            const float2 q = ms[t];
            ms[t].x = expf(lg[(size_t)t * C + ext[2 * i + 1]] - q.x) / q.y;
        }
    }
    __threadfence_block();
    __syncthreads();
    // ---- phase 3: per symbol, the mean over its span
    if (tid < L) {
        float c = 0.f;
        if (tid < len) {
            const int a = min(max(st[tid], 0), Tn), e = min(max(en[tid], a), Tn);
            double acc = 0.0;
            for (int t = a; t < e; ++t) acc += (double)ms[t].x;
            if (e > a) c = (float)(acc / (double)(e - a));
        }
        cf[tid] = c;
    }
}

template <bool VL>
static int launch_ctc_align_t(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank, void* ws, int* frame_pos, int* start,
                              int* end, float* conf, float* score, const int* frame_len, hipStream_t s) {
    const int ns = ctc_ns(L);
    if (ns < 1 || ns > 8 || C > 64) { ishara_set_error("ctc_align: L=%d (max 255) or C=%d (max 64) unsupported", L, C); return -1; }
    const bool fast = ctc_align_bp_in_lds(T, L);
    const size_t shmem = align_lds_bytes(T, L, fast);
#define ALIGN_L(NS, F) do { \
        if (shmem + ALIGN_LDS_STATIC > ALIGN_LDS_DEFAULT) {      /* more than every launch is granted: raise the kernel's limit once */ \
            static bool raised = false; \
            if (!raised) { \
                if (hipFuncSetAttribute(reinterpret_cast<const void*>(&ctc_align_kernel<NS, F, VL>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                        (int)(ALIGN_LDS_MAX - ALIGN_LDS_STATIC)) != hipSuccess) { \
                    ishara_set_error("ctc_align: cannot reserve %zu bytes of LDS", shmem); return -2; \
                } \
                raised = true; \
            } \
        } \
        hipLaunchKernelGGL((ctc_align_kernel<NS, F, VL>), dim3(B), dim3(256), shmem, s, logits, labels, T, C, L, blank, reinterpret_cast<uint16_t*>(ws), \
                           frame_pos, start, end, conf, score, frame_len); \
    } while (0)
#define ALIGN_NS(NS) do { if (fast) ALIGN_L(NS, true); else ALIGN_L(NS, false); } while (0)
    switch (ns) { case 1: ALIGN_NS(1); break; case 2: ALIGN_NS(2); break; case 3: ALIGN_NS(3); break; case 4: ALIGN_NS(4); break;
                  case 5: ALIGN_NS(5); break; case 6: ALIGN_NS(6); break; case 7: ALIGN_NS(7); break; default: ALIGN_NS(8); break; }
#undef ALIGN_NS
#undef ALIGN_L
    return launch_rc();
}
int launch_ctc_align(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank, void* ws, int* frame_pos, int* start,
                     int* end, float* conf, float* score, hipStream_t s) {
    return launch_ctc_align_t<false>(logits, labels, B, T, C, L, blank, ws, frame_pos, start, end, conf, score, nullptr, s);
}
int launch_ctc_align_len(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank, void* ws, int* frame_pos, int* start,
                         int* end, float* conf, float* score, const int* frame_len, hipStream_t s) {
    return launch_ctc_align_t<true>(logits, labels, B, T, C, L, blank, ws, frame_pos, start, end, conf, score, frame_len, s);
}
