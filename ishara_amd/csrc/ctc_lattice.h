// The CTC forward / backward lattice arithmetic, stated once for the kernels that run it: ctc_kernel (ctc.hip: loss and gradient),
// ctc_score_kernel (ctc_score.hip: the alpha chain alone) and ng_lattice_kernel / ng_grad_kernel (ctc_nbest_grad.hip).  Their contracts
// need equal bits (ishara_ctc_score_nbest == float32(-nll) of ishara_ctc_loss_ex; ishara_ctc_nbest_grad at N = 1, coef = 1 == ctc_kernel's
// dlogits and dlb), and they get them by calling the same functions.
//
// The arrangement: the S = 2 len + 1 lattice states of a sample live in the registers of one wave, state s = lane + 64 k (k < NS).  NK is the
// COMPILE-TIME number of occupied registers per lane (1: up to 31 symbols, 2: up to 63), so that the per-k loops are straight-line code;
// NK = 0 keeps the run-time count nk = ceil(S / 64).  The s-1 / s-2 neighbours come from lanes l-1 / l-2 by a rotation; lanes 0 (and 1)
// take them from lanes 63 (and 62) of register k - 1.  Everything here is force-inlined into its caller, which keeps what is its own: the
// refusals, the result writes and the NK dispatch.
#pragma once
#include "kernels.h"

#define CTC_NEG (-1e30)
// log(e^a + e^b + e^c) with the running state in fp64 and the transcendentals in fp32: the lattice values reach ~-1700 at
// T=384 where an fp32 ulp is 1.2e-4 and the drift over T frames reaches 1e-3 relative in the posteriors; fp64 add/max keeps
// the drift at the 1e-6 level while exp/log only ever see small-magnitude differences.  (A scaled PROBABILITY-space
// recursion is not an option: the state vector of one frame spans > 250 decades on random logits, tools/ notes in DESIGN.md.)
DEVI double lse3(double a, double b, double c) {
    // branch-free: with all three terms dead (m = CTC_NEG) the exponentials are exp(0) and the result is discarded by the select — an early
    // return was an exec-mask branch on the recursions' dependency chain
    const double m = fmax(a, fmax(b, c));
    const float sum = __expf((float)(a - m)) + __expf((float)(b - m)) + __expf((float)(c - m));
    const double r = m + (double)__logf(sum);
    return m <= -1e29 ? CTC_NEG : r;
}

// logsumexp of one row of C logits: lse[t] of every kernel (and so the softmax each of them subtracts from)
DEVI float ctc_row_lse(const float* __restrict__ row, int C) {
    float m = -1e30f;
    for (int c = 0; c < C; ++c) m = fmaxf(m, row[c]);
    float a = 0.f;
    for (int c = 0; c < C; ++c) a += expf(row[c] - m);
    return m + logf(a);
}

static inline int ctc_ns(int L) { return (2 * L + 1 + 63) / 64; }            // lattice states per lane of the recursion wave

// ---- hypothesis rows ------------------------------------------------------------------------------------------
enum { CTC_HYP_DEAD = 1, CTC_HYP_NOALIGN = 2, CTC_HYP_SYMBOL = 4, CTC_HYP_LONG = 8 };      // mirrored in ishara_amd/rescore.py
// the status of one hypothesis (len symbols of a row Th wide) against Tn frames, the first bit that applies; 0: it has an alignment as far
// as its symbols and repeats tell.  Wave-collective.  max_len: a tighter length limit than the kernels' own 255
DEVI int ctc_hyp_status(const int* __restrict__ hyp, int len, int Th, int C, int blank, int Tn, int lane, int max_len = 255) {
    if (len < 0) return CTC_HYP_DEAD;
    if (len > Th || len > 255 || len > max_len) return CTC_HYP_LONG;
    int bad = 0, rep = 0;
    for (int i0 = 0; i0 < len; i0 += 64) {
        const int i = i0 + lane;
        const int v = i < len ? hyp[i] : 0;
        const bool ok = v >= 0 && v < C && v != blank;
        bad |= (i < len && !ok) ? 1 : 0;
        rep += (i < len && i > 0 && v == hyp[i - 1]) ? 1 : 0;
    }
    bad = __any(bad);
    rep = __popcll(__ballot(rep & 1)) + 2 * __popcll(__ballot(rep & 2)) + 4 * __popcll(__ballot(rep & 4));      // rep <= 4 per lane
    if (bad) return CTC_HYP_SYMBOL;
    return (Tn < 1 || Tn < len + rep) ? CTC_HYP_NOALIGN : 0;          // Tn = 0: no frames, not even for the empty hypothesis
}
// the symbol of lattice state s of a checked hypothesis: odd states carry symbol s >> 1 (< len), the others the blank
DEVI int ctc_hyp_symbol(const int* __restrict__ hyp, int S, int blank, int s) { return (s < S && (s & 1)) ? hyp[s >> 1] : blank; }

// ---- the states of a lane -------------------------------------------------------------------------------------
// the set-up of a chain that reads its label from memory (ctc_score_kernel; ctc_lattice_waves below reads an LDS row by state).
// sym(i): symbol i of the label (0 <= i < len), the symbol of the odd state 2 i + 1; the even states carry the blank.  act: the state
// exists; skip_bw: the transition s-2 -> s exists.
template <int NK, int NS, typename Sym>
DEVI void ctc_states(Sym sym, int S, int blank, int lane, int (&my)[NS], bool (&act)[NS], bool (&skip_bw)[NS]) {
#pragma unroll
    for (int k = 0; k < (NK ? NK : NS); ++k) {
        const int s = lane + 64 * k;
        act[k] = s < S;
        const bool odd = act[k] && (s & 1);
        my[k] = odd ? sym(s >> 1) : blank;
        const int prev = (odd && s >= 3) ? sym((s >> 1) - 1) : blank;
        skip_bw[k] = act[k] && s >= 2 && my[k] != blank && my[k] != prev;
    }
}
// ---- the emission pipeline: U frames are gathered a group ahead of the chain ---------------------------------------
// RAW logits of frames t0, t0 + dir, .., t0 + (U - 1) dir (loads only: subtracting lse here made hipcc wait for the loads right
// after issuing them)
template <int NK, int U, int NS>
DEVI void ctc_gather(const float* __restrict__ lg, int C, int Tn, int nk, const int (&my)[NS], int t0, int dir, float (&dst)[U][NS]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int t = min(max(t0 + dir * u, 0), Tn - 1);
#pragma unroll
        for (int k = 0; k < (NK ? NK : NS); ++k)
            if (NK != 0 || k < nk) dst[u][k] = lg[(size_t)t * C + my[k]];
    }
}
// emission log-probabilities of a gathered group, one group later: the loads have landed by then (the empty asm keeps the
// subtraction from being scheduled up to the loads)
template <int NK, int U, int NS>
DEVI void ctc_settle(const float* lse, int Tn, int nk, int t0, int dir, float (&src)[U][NS], float (&dst)[U][NS]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const float ls = lse[min(max(t0 + dir * u, 0), Tn - 1)];
#pragma unroll
        for (int k = 0; k < (NK ? NK : NS); ++k)
            if (NK != 0 || k < nk) { asm volatile("" : "+v"(src[u][k])); dst[u][k] = src[u][k] - ls; }
    }
}

// ---- alpha ----------------------------------------------------------------------------------------------------
// frame 0: only states 0 and 1 are alive (ctc_score_kernel; ctc_lattice_waves below writes the same expression in the loop that also
// stores the row)
template <int NK, int NS>
DEVI void ctc_alpha_init(const float* __restrict__ lg, const float* lse, int len, int lane, const int (&my)[NS], const bool (&act)[NS], double (&a)[NS]) {
#pragma unroll
    for (int k = 0; k < (NK ? NK : NS); ++k) {
        const int s = lane + 64 * k;
        a[k] = (act[k] && (s == 0 || (s == 1 && len > 0))) ? (double)(lg[my[k]] - lse[0]) : CTC_NEG;
    }
}
// one frame of an alpha chain that keeps no lattice (ctc_score_kernel): a = alpha_{t-1} on entry, alpha_t on return; em: the frame's
// emission log-probabilities.  The k loop runs from the top register down and writes a[k] in place: a[k]'s rotations are taken before it
// is overwritten and handed down to k - 1's step, so the rotations and new values are four scalars: half the registers at NS = 8
template <int NK, int NS>
DEVI void ctc_alpha_step_inplace(double (&a)[NS], const bool (&act)[NS], const bool (&skip_bw)[NS], const float (&em)[NS], int nk, int lane) {
    constexpr int KM = NK ? NK : NS;
    double top = a[0];
#pragma unroll
    for (int k = 1; k < KM; ++k)
        if (NK != 0 || k < nk) top = a[k];
    double up1 = __shfl(top, (lane + 63) & 63, 64), up2 = __shfl(top, (lane + 62) & 63, 64);      // the rotations of the top register
#pragma unroll
    for (int k = KM - 1; k >= 0; --k)
        if (NK != 0 || k < nk) {
            double lo1 = CTC_NEG, lo2 = CTC_NEG;                                                       // the rotations of register k - 1
            if (k >= 1) { lo1 = __shfl(a[k >= 1 ? k - 1 : 0], (lane + 63) & 63, 64); lo2 = __shfl(a[k >= 1 ? k - 1 : 0], (lane + 62) & 63, 64); }
            const double a1 = lane >= 1 ? up1 : lo1;
            const double a2 = lane >= 2 ? up2 : lo2;
            double v = act[k] ? lse3(a[k], a1, skip_bw[k] ? a2 : CTC_NEG) : CTC_NEG;
            if (v > -1e29) v += (double)em[k];
            a[k] = v;
            up1 = lo1; up2 = lo2;
        }
}
// log p(y | x) = logsumexp(alpha[S-1], alpha[S-2]): both live in (at most two) lanes; reduce max then sum over the wave
template <int NK, int NS>
DEVI double ctc_alpha_final(const double (&a)[NS], int S, int len, int lane) {
    double cand = CTC_NEG, cand2 = CTC_NEG;
#pragma unroll
    for (int k = 0; k < (NK ? NK : NS); ++k) {
        const int s = lane + 64 * k;
        if (s == S - 1) cand = a[k];
        if (s == S - 2 && len > 0) cand2 = a[k];
    }
    double m = fmax(cand, cand2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    float e = 0.f;
    if (m > -1e29) e = ((cand > -1e29) ? __expf((float)(cand - m)) : 0.f) + ((cand2 > -1e29) ? __expf((float)(cand2 - m)) : 0.f);
    e = wave_sum(e);
    return m > -1e29 ? m + (double)__logf(e) : CTC_NEG;
}

// ---- the two recursion waves of a lattice that is kept (ctc_kernel, ng_lattice_kernel) ----------------------------------------
// wave 0 runs the alpha chain and stores alpha_t[s] to Gw, wave 1 the beta chain (with emission: bt = beta_{t+1}) and stores
// bsum_t[s] = logsumexp of the successors' betas to Hw, concurrently on two SIMDs; rows SPw doubles apart, only the occupied registers
// written.  ext: the extended label row in LDS (64 NS entries, blank on the even states and past S).  done(logp): called by wave 0 with
// log p(y | x); the result writes are the caller's.
// The alpha step here takes the rotations of every register first (three arrays of NS doubles): ctc_alpha_step_inplace in its place
// costs ctc_kernel<5> six registers across an occupancy step and ng_lattice_kernel<2> 0.3 % of its time
template <int NS, int NK, typename Done>
DEVI void ctc_lattice_waves(const float* __restrict__ lg, const float* lse, const int* ext, int S, int len, int Tn, int C, int blank, double* __restrict__ Gw,
                            double* __restrict__ Hw, int SPw, int lane, int wave, Done done) {
    constexpr int KM = NK ? NK : NS;
    const int nk = NK ? NK : ((S + 63) >> 6);
    bool act[NS], skip_bw[NS], skip_fw[NS];
    int my[NS];
    // the set-up read from ext[] by state, skip_fw (s -> s+2) with it: through ctc_states' label accessor the same values cost
    // ishara_ctc_loss 0.2 % and ishara_ctc_nbest_grad 0.5 % of their time
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        const int s = lane + 64 * k;
        my[k] = ext[s];
        act[k] = s < S;
        skip_bw[k] = act[k] && s >= 2 && my[k] != blank && my[k] != ext[s >= 2 ? s - 2 : 0];       // s-2 -> s
        skip_fw[k] = s + 2 < S && ext[s + 2 < S ? s + 2 : s] != blank && ext[s + 2 < S ? s + 2 : s] != my[k];      // s -> s+2
    }
    float em[8][NS], emn[8][NS];
    const auto gather = [&](int t0, int dir, float (&dst)[8][NS]) { ctc_gather<NK>(lg, C, Tn, nk, my, t0, dir, dst); };
    const auto settle = [&](int t0, int dir, float (&src)[8][NS], float (&dst)[8][NS]) { ctc_settle<NK>(lse, Tn, nk, t0, dir, src, dst); };
    if (wave == 0) {
        // ---- alpha ----
        double a[NS];
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            const int s = lane + 64 * k;
            a[k] = (act[k] && (s == 0 || (s == 1 && len > 0))) ? (double)(lg[my[k]] - lse[0]) : CTC_NEG;
            if (NK != 0 || k < nk) Gw[s] = a[k];
        }
        gather(1, 1, emn);
        settle(1, 1, emn, em);
        for (int t0 = 1; t0 < Tn; t0 += 8) {
            if (t0 + 8 < Tn) gather(t0 + 8, 1, emn);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = t0 + u;
                if (t < Tn) {
                    double r1[NS], r2[NS], n[NS];
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (NK != 0 || k < nk) { r1[k] = __shfl(a[k], (lane + 63) & 63, 64); r2[k] = __shfl(a[k], (lane + 62) & 63, 64); }
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (NK != 0 || k < nk) {
                            const double a1 = lane >= 1 ? r1[k] : (k >= 1 ? r1[k >= 1 ? k - 1 : 0] : CTC_NEG);
                            const double a2 = lane >= 2 ? r2[k] : (k >= 1 ? r2[k >= 1 ? k - 1 : 0] : CTC_NEG);
                            double v = act[k] ? lse3(a[k], a1, skip_bw[k] ? a2 : CTC_NEG) : CTC_NEG;
                            if (v > -1e29) v += (double)em[u][k];
                            n[k] = v;
                        }
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (NK != 0 || k < nk) { a[k] = n[k]; Gw[(size_t)t * SPw + lane + 64 * k] = n[k]; }
                }
            }
            if (t0 + 8 < Tn) settle(t0 + 8, 1, emn, em);
        }
        done(ctc_alpha_final<NK>(a, S, len, lane));
    } else {
        // ---- beta (with emission): bt = beta_{t+1}; stores bsum_t[s] = logsumexp of the successors' betas ----
        double bt[NS];
#pragma unroll
        for (int k = 0; k < KM; ++k) bt[k] = CTC_NEG;
        gather(Tn - 1, -1, emn);
        settle(Tn - 1, -1, emn, em);
        for (int tb = Tn - 1; tb >= 0; tb -= 8) {
            if (tb - 8 >= 0) gather(tb - 8, -1, emn);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int t = tb - u;
                if (t >= 0) {
                    double bsum[NS];
                    if (t == Tn - 1) {
#pragma unroll
                        for (int k = 0; k < KM; ++k) {
                            const int s = lane + 64 * k;
                            bsum[k] = (act[k] && (s == S - 1 || (s == S - 2 && len > 0))) ? 0.0 : CTC_NEG;
                        }
                    } else {
                        double d1[NS], d2[NS];
#pragma unroll
                        for (int k = 0; k < KM; ++k)
                            if (NK != 0 || k < nk) { d1[k] = __shfl(bt[k], (lane + 1) & 63, 64); d2[k] = __shfl(bt[k], (lane + 2) & 63, 64); }
#pragma unroll
                        for (int k = 0; k < KM; ++k)
                            if (NK != 0 || k < nk) {
                                // successors s+1 / s+2: lanes 63 (and 62) take them from lanes 0 (and 1) of the next k (absent: no state)
                                const bool nx = k + 1 < KM && k + 1 < nk;
                                const double b1 = lane <= 62 ? d1[k] : (nx ? d1[k + 1 < KM ? k + 1 : k] : CTC_NEG);
                                const double b2 = lane <= 61 ? d2[k] : (nx ? d2[k + 1 < KM ? k + 1 : k] : CTC_NEG);
                                bsum[k] = act[k] ? lse3(bt[k], b1, skip_fw[k] ? b2 : CTC_NEG) : CTC_NEG;
                            }
                    }
#pragma unroll
                    for (int k = 0; k < KM; ++k)
                        if (NK != 0 || k < nk) {
                            Hw[(size_t)t * SPw + lane + 64 * k] = bsum[k];
                            bt[k] = bsum[k] > -1e29 ? bsum[k] + (double)em[u][k] : CTC_NEG;
                        }
                }
            }
            if (tb - 8 >= 0) settle(tb - 8, -1, emn, em);
        }
    }
}

// ---- state posteriors -> class posteriors by LDS scatter-add --------------------------------------------------------
// (one frame per wave at a time: O(T*S) work; a (frame, class) thread looping over the states was O(T*C*S) and took longer than both
// recursions.  The callers load the rows al / bs of U frames first, so that they are in flight together.)
// one frame: every live state adds exp(alpha + bsum - logp) to the class sym(k) of its state lane + 64 k
template <int NS, typename Sym>
DEVI void ctc_post_add(float* cls, Sym sym, int S, double logp, const double (&al)[NS], const double (&bs)[NS], int lane) {
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const int s = lane + 64 * k;
        if (s < S && al[k] > -1e29 && bs[k] > -1e29 && logp > -1e29) atomicAdd(&cls[sym(k)], __expf((float)(al[k] + bs[k] - logp)));
    }
}

// the bf16 copy of a gradient row held one class per lane, zero padded to 128 classes (MFMA operand of the classifier's dgrad / wgrad);
// row: the 64 words of the row
DEVI void store_dlb_row(uint32_t* __restrict__ row, float gv, int lane) {
    const float lo = __shfl(gv, (2 * lane) & 63, 64), hi = __shfl(gv, (2 * lane + 1) & 63, 64);
    typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
    bf2 pk; pk[0] = (__bf16)(lane < 32 ? lo : 0.f); pk[1] = (__bf16)(lane < 32 ? hi : 0.f);
    row[lane] = __builtin_bit_cast(uint32_t, pk);
}
