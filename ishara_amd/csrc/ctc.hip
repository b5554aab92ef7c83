// CTC loss + gradient (conv-hybrid-model.ipynb c6:1-13 -> tf.nn.ctc_loss semantics with
// blank = last class, logit_length = T) and the greedy decoder (c8:4-12).
//
// One workgroup per sample; the lattice has S = 2*len+1 <= 2L+1 states (see ctc_scaled_kernel).
//
// Samples without an alignment.  A sample is INFEASIBLE when T < len + repeats (no path through the lattice) or when its label row holds a
// value outside [0, C).  For such a sample nll[b] = 1e30 (the sentinel: >= 1e29), every posterior is zero, so dlogits[b] = grad_scale *
// softmax(logits[b]) (finite) and dlb its bf16 copy; an out-of-range label reads as blank (no read outside the logits row, no LDS add outside
// the class row).  The other samples of the batch are computed exactly as if that sample were not there (one workgroup per sample, nothing
// shared): their nll, dlogits and dlb are bit-identical.  The caller decides what an nll of 1e30 means (tf.nn.ctc_loss returns inf there).
#include <type_traits>
#include "ctc_lattice.h"                                // the lattice arithmetic (lse3, the state set-up, the emission pipeline, the frame steps)

// LDS of one workgroup: lse[T] and ext[64 NS] are requested at launch; cls (4 KiB), s_logp, s_len and s_bad are static.  The kernel is launched
// without a raised dynamic-LDS attribute, so static + dynamic stay within the 64 KiB every HIP launch is granted.
static constexpr size_t CTC_LDS_STATIC = 4 * 4 * 64 * sizeof(float) + 2 * sizeof(double), CTC_LDS_LAUNCH = 65536;
size_t ctc_lds_bytes(int T, int L) { return (size_t)T * sizeof(float) + (size_t)64 * ctc_ns(L) * sizeof(int); }
size_t ctc_lds_limit() { return CTC_LDS_LAUNCH - CTC_LDS_STATIC; }
size_t ctc_workspace_floats(int B, int T, int L) { return 4 * (size_t)B * T * 64 * ctc_ns(L); }   // two fp64 lattices [B][T][64*NS]: alpha, beta sums

// ---------------------------------------------------------------------------------------------------------------
// One 256-thread workgroup per sample:
//   phase 0 (all threads)  lse[t] = logsumexp(logits[t]); extended label sequence
//   phase 1 (wave 0)       alpha recursion in log space: the S = 2*len+1 states live in REGISTERS, state s = lane + 64 k;
//                          only the ceil(S/64) occupied k are computed; the s-1 / s-2 neighbours come from the previous
//                          lanes by two rotations per frame and k.  No barrier and no LDS on the dependency chain (the previous kernel
//                          spent a workgroup barrier and an L2 round trip per frame: 0.9 ms at T=384); the emission
//                          log-probabilities are gathered 8 frames ahead of the chain.
//   phase 1' (wave 1)      beta recursion the same way, CONCURRENTLY with alpha on another SIMD (the two chains are
//                          independent); it stores bsum_t[s] = log sum of the successors' betas
//   phase 2 (all threads)  state posteriors exp(alpha + bsum - logp) scatter-added to classes in LDS, one frame per wave at
//                          a time; dlogits = grad_scale * (softmax - posterior)
// ---------------------------------------------------------------------------------------------------------------
//
// VL (per-sample frame counts, ishara_ctc_loss_ex): Ts, the buffer's T, stays the stride of every row offset and of the LDS layout; the sample's
// own count Tn = frame_len[b] takes every other role, so the sample computes what a one-sample launch at T = Tn on logits[b, :Tn] computes,
// and rows t >= Tn are not read.  dlogits[b, t >= Tn] = +0.  A frame_len[b] outside [1, Ts] is never an index or a bound: the sample has no
// frames (nll = 1e30, every dlogits row +0).  sample_scale[b] multiplies grad_scale; zero_inf makes an infeasible sample's gradient +0.
// With VL = false Tn is Ts and the three extra arguments are not read: the code of the fixed-T entry points.
template <int NS, bool VL>
__global__ __launch_bounds__(256) void ctc_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                  int Ts, int C, int L, int blank, float* __restrict__ nll,
                                                  float* __restrict__ dlogits, float grad_scale, double* __restrict__ ws,
                                                  uint32_t* __restrict__ dlb, const int* __restrict__ frame_len,
                                                  const float* __restrict__ sample_scale, int zero_inf) {
    constexpr int SP = 64 * NS;
    extern __shared__ float shf[];
    float* lse = shf;                                   // [Ts]
    int* ext = reinterpret_cast<int*>(lse + Ts);        // [SP]
    __shared__ int s_len, s_bad;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    int Tn = Ts;
    if (VL) {
        if (frame_len) Tn = frame_len[b];
        if (Tn < 1 || Tn > Ts) {                        // no frames (workgroup-uniform): the sentinel and a zero gradient
            if (tid == 0) nll[b] = 1e30f;
            if (dlogits)
                for (size_t i = tid; i < (size_t)Ts * C; i += 256) dlogits[(size_t)b * Ts * C + i] = 0.f;
            return;
        }
        if (sample_scale) grad_scale *= sample_scale[b];
    }
    const float* lg = logits + (size_t)b * Ts * C;
    const int64_t* lab = labels + (size_t)b * L;
    double* Gw = ws + (size_t)b * 2 * Ts * SP;          // [Ts][SP] alpha
    double* Hw = Gw + (size_t)Ts * SP;                  // [Ts][SP] bsum
    __shared__ double s_logp;

    // a label outside [0, C) makes the sample infeasible (header comment); it enters ext as blank, so nothing below indexes with it
    if (tid == 0) {
        int n = 0, bad = 0;
        for (int i = 0; i < L; ++i) { const int64_t v = lab[i]; n += (v != blank) ? 1 : 0; bad |= (v < 0 || v >= C) ? 1 : 0; }
        s_len = n; s_bad = bad;
    }
    for (int t = tid; t < Tn; t += 256) lse[t] = ctc_row_lse(lg + (size_t)t * C, C);
    for (int s = tid; s < SP; s += 256) {
        const int64_t v = (s < 2 * L + 1 && (s & 1)) ? lab[s >> 1] : (int64_t)blank;
        ext[s] = (v < 0 || v >= C) ? blank : (int)v;
    }
    __syncthreads();
    const int len = s_len, S = 2 * len + 1;

    // The recursions, instantiated for a COMPILE-TIME number NK of occupied state registers per lane (1: labels of up to 31 symbols, 2: up to 63)
    // so that the per-k loops are straight-line code; NK = 0 keeps the run-time count (longer labels).  The block picks its instantiation below.
    auto recursions = [&](auto nkc) {
        ctc_lattice_waves<NS, decltype(nkc)::value>(lg, lse, ext, S, len, Tn, C, blank, Gw, Hw, SP, lane, tid >> 6, [&](double lp) {
            const double logp = s_bad ? CTC_NEG : lp;
            if (lane == 0) { nll[b] = (float)(-logp); s_logp = logp; }
        });
    };
    if (tid < 128) {
        const int nkb = (S + 63) >> 6;
        if (NS >= 2 && nkb == 1) recursions(std::integral_constant<int, 1>{});
        else if (NS >= 3 && nkb == 2) recursions(std::integral_constant<int, 2>{});
        else recursions(std::integral_constant<int, 0>{});
    }
    __threadfence_block();
    __syncthreads();
    // ---- phase 3: state posteriors -> class posteriors by LDS scatter-add, then the gradient
    if (dlogits) {
        // four frames of a wave in flight together: the loop used to wait out one L2 round trip per frame (96 dependent trips per wave)
        constexpr int U = 4;
        __shared__ float cls[4][U][64];
        const double logp = s_logp;
        float* dl = dlogits + (size_t)b * Ts * C;
        const int wv = tid >> 6;
        if (VL) {
            const bool dead = zero_inf && !(logp > -1e29);        // zero_infinity: an infeasible sample's rows are +0 as well
            const int t0 = dead ? 0 : Tn;
            for (size_t i = (size_t)t0 * C + tid; i < (size_t)Ts * C; i += 256) dl[i] = 0.f;
            if (dead) return;
        }
        for (int t0 = wv; t0 < Tn; t0 += 4 * U) {
            double al[U][NS], bs[U][NS];
            float lgv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = min(t0 + 4 * u, Tn - 1);
                cls[wv][u][lane] = 0.f;
                const double* ga = Gw + (size_t)t * SP;
                const double* gb = Hw + (size_t)t * SP;
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const int s = lane + 64 * k;              // strided: coalesced 512-byte reads of the lattice rows
                    al[u][k] = s < S ? ga[s] : CTC_NEG; bs[u][k] = s < S ? gb[s] : CTC_NEG;
                }
                lgv[u] = lane < C ? lg[(size_t)t * C + lane] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int t = t0 + 4 * u;
                if (t >= Tn) continue;                        // wave-uniform
                ctc_post_add(cls[wv][u], [&](int k) { return ext[lane + 64 * k]; }, S, logp, al[u], bs[u], lane);
                float gv = 0.f;
                if (lane < C) {
                    const float sm = expf(lgv[u] - lse[t]);
                    gv = grad_scale * (sm - cls[wv][u][lane]);
                    dl[(size_t)t * C + lane] = gv;
                }
                if (dlb) store_dlb_row(dlb + ((size_t)b * Ts + t) * 64, gv, lane);
            }
        }
    }
}

#define CTC_L(NS, VL, FL, SS, ZI) hipLaunchKernelGGL((ctc_kernel<NS, VL>), dim3(B), dim3(256), shmem, s, logits, labels, T, C, L, blank, nll, dlogits, grad_scale, reinterpret_cast<double*>(ws), reinterpret_cast<uint32_t*>(dlb), FL, SS, ZI)
#define CTC_NS(VL, FL, SS, ZI) switch (ns) { case 1: CTC_L(1, VL, FL, SS, ZI); break; case 2: CTC_L(2, VL, FL, SS, ZI); break; case 3: CTC_L(3, VL, FL, SS, ZI); break; \
                  case 4: CTC_L(4, VL, FL, SS, ZI); break; case 5: CTC_L(5, VL, FL, SS, ZI); break; case 6: CTC_L(6, VL, FL, SS, ZI); break; \
                  case 7: CTC_L(7, VL, FL, SS, ZI); break; default: CTC_L(8, VL, FL, SS, ZI); break; }
int launch_ctc(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank,
               float* nll, float* dlogits, float grad_scale, float* ws, hipStream_t s, void* dlb) {
    if (2 * L + 1 > 512 || C > 64) { ishara_set_error("ctc: L=%d (max 255) or C=%d (max 64) unsupported", L, C); return -1; }
    const int ns = ctc_ns(L);
    const size_t shmem = ctc_lds_bytes(T, L);
    CTC_NS(false, (const int*)nullptr, (const float*)nullptr, 0)
    return launch_rc();
}
// per-sample frame counts (the VL instantiations): frame_len [B] int32 and sample_scale [B] f32 on the device, either may be NULL
int launch_ctc_len(const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank, float* nll, float* dlogits,
                   float grad_scale, float* ws, const int* frame_len, const float* sample_scale, int zero_inf, hipStream_t s) {
    if (2 * L + 1 > 512 || C > 64) { ishara_set_error("ctc: L=%d (max 255) or C=%d (max 64) unsupported", L, C); return -1; }
    const int ns = ctc_ns(L);
    const size_t shmem = ctc_lds_bytes(T, L);
    void* dlb = nullptr;
    CTC_NS(true, frame_len, sample_scale, zero_inf)
    return launch_rc();
}
#undef CTC_NS
#undef CTC_L

__global__ void mean_kernel(const float* __restrict__ v, float* __restrict__ out, int n, float scale) {
    __shared__ float red[4];
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) a += v[i];
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (red[0] + red[1] + red[2] + red[3]) * scale;
}
int launch_mean(const float* v, float* out, int n, float scale, hipStream_t s) {
    hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(256), 0, s, v, out, n, scale);
    return launch_rc();
}

// greedy decode: argmax per frame (first max on ties), keep x[i] (i <= T-2) where
// x[i] != x[i+1], drop blanks (the reference never emits the final run, c8:7-9).
// VL: the sample has Tn = frame_len[b] frames of the buffer's Ts (the stride, and the width of the -1 padding); outside [1, Ts]: none.
template <bool VL>
__global__ __launch_bounds__(256) void greedy_decode_kernel(const float* __restrict__ logits, int Ts, int C, int blank,
                                                            int* __restrict__ out_idx, int* __restrict__ out_len,
                                                            const int* __restrict__ frame_len) {
    extern __shared__ int shi[];   // am[Ts]
    int* am = shi;
    __shared__ int s_wcnt[4], s_base;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    int Tn = Ts;
    if (VL && frame_len) { Tn = frame_len[b]; if (Tn < 1 || Tn > Ts) Tn = 0; }
    const float* lg = logits + (size_t)b * Ts * C;
    for (int t = tid; t < Tn; t += blockDim.x) {
        float best = lg[(size_t)t * C];
        int bi = 0;
        for (int c0 = 0; c0 < C; c0 += 16) {       // 16 loads in flight, then the (ordered: first max wins) comparisons
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = lg[(size_t)t * C + min(c0 + u, C - 1)];
#pragma unroll
            for (int u = 0; u < 16; ++u) if (c0 + u < C && v[u] > best) { best = v[u]; bi = c0 + u; }
        }
        am[t] = bi;
    }
    if (tid == 0) s_base = 0;
    __syncthreads();
    // kept frames go out in order: positions by a ballot prefix, 256 frames per round (a serial scan by one thread was 18 us of the
    // kernel's 25 at T = 384)
    for (int t0 = 0; t0 < Tn; t0 += 256) {
        const int t = t0 + tid;
        const int keep = (t + 1 < Tn && am[t] != am[t + 1] && am[t] != blank) ? 1 : 0;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcnt[wid] = __popcll(bal);
        __syncthreads();
        int off = s_base;
        for (int w = 0; w < wid; ++w) off += s_wcnt[w];
        if (keep) out_idx[(size_t)b * Ts + off + before] = am[t];
        __syncthreads();
        if (tid == 0) s_base += s_wcnt[0] + s_wcnt[1] + s_wcnt[2] + s_wcnt[3];
        __syncthreads();
    }
    const int n = s_base;
    if (tid == 0) out_len[b] = n;
    for (int t = n + tid; t < Ts; t += blockDim.x) out_idx[(size_t)b * Ts + t] = -1;      // the -1 padding (was a fill launch of its own)
}

int launch_greedy_decode(const float* logits, int B, int T, int C, int blank, int* out_idx, int* out_len, hipStream_t s) {
    hipLaunchKernelGGL(greedy_decode_kernel<false>, dim3(B), dim3(256), T * sizeof(int), s, logits, T, C, blank, out_idx, out_len, (const int*)nullptr);
    return launch_rc();
}
int launch_greedy_decode_len(const float* logits, int B, int T, int C, int blank, int* out_idx, int* out_len, const int* frame_len, hipStream_t s) {
    hipLaunchKernelGGL(greedy_decode_kernel<true>, dim3(B), dim3(256), T * sizeof(int), s, logits, T, C, blank, out_idx, out_len, frame_len);
    return launch_rc();
}
