// The weights of minimum-risk (MWER) training over an n-best list (ishara_mwer_weights; contract in include/ishara_hip.h, host definition in
// ishara_amd/mwer.py): every slot's edit distance to the target, the posterior of the list renormalised over its live slots, the expected
// distance (the risk) and coef[b, n] = d risk / d nll_n, which ishara_ctc_nbest_grad takes as it is.
//
// One wave per clip, lane = slot.  The distance is edit_distance.h's myers: Hyyro's bit-vector form of Myers' algorithm, one 64-bit word, the
// TARGET as the pattern (<= 64 symbols), the hypothesis as the text; the match masks peq[c] by one ballot per class.  No fallback phrase.
// The sums run over the slots in ascending order from +0 in every lane, each step one fp32 operation without FMA contraction.
// Duplicate strings are not merged: the prefix beam search emits distinct prefixes.  No workspace, no atomics, graph-capturable.
#include "edit_distance.h"

__global__ __launch_bounds__(64) void mwer_weights_kernel(const int* __restrict__ hyp_idx, const int* __restrict__ hyp_len, const float* __restrict__ logp,
                                                          const int* __restrict__ status, int N, int Th, const int* __restrict__ targets, int L,
                                                          const float* __restrict__ inv_temp, int mode, int* __restrict__ dist_out,
                                                          float* __restrict__ post_out, float* __restrict__ risk_out, float* __restrict__ coef_out,
                                                          int* __restrict__ tlen_out) {
#pragma clang fp contract(off)                          // one rounding per operation: hipcc would fuse a * b + c, through __fmul_rn / __fadd_rn too
                                                        // (plain operators in its headers, see awp.hip's awp_step): plain operators under the pragma
    __shared__ uint64_t s_peq[64];
    __shared__ int s_tgt[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    // ---- the target: the symbols before the first 59, its match masks
    const int nb = target_prep(targets + (size_t)b * L, L, lane, s_tgt, s_peq);
    __syncthreads();
    // ---- the slot of this lane
    const size_t slot = (size_t)b * N + (lane < N ? lane : 0);
    int len = lane < N ? hyp_len[slot] : -1;
    len = len > Th ? Th : len;                          // never read past the row
    const float lp = lane < N ? logp[slot] : 0.f;
    const int stv = (lane < N && status) ? status[slot] : 0;
    const bool live = lane < N && len >= 0 && stv == 0 && fabsf(lp) < INFINITY;       // a NaN compares false
    const int* text = hyp_idx + slot * Th;
    const int d = live ? myers(nb, [&](int k) { return match_mask(s_peq, s_tgt, nb, text[k]); }, len) : -1;
    const float it = inv_temp ? inv_temp[0] : 1.f;
    float W = (float)d;
    if (mode == 1) W = W / (float)(nb > 1 ? nb : 1);
    float mx = live ? lp : -INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const unsigned long long lv = __ballot(live);
    float e = 0.f;
    if (live) { const float dx = lp - mx; const float x = dx * it; e = expf(x); }
    float tot = 0.f;
    for (int n = 0; n < N; ++n) {
        const float en = __shfl(e, n, 64);
        if ((lv >> n) & 1ull) tot = tot + en;
    }
    const float p = live ? e / tot : 0.f;
    float risk = 0.f;
    for (int n = 0; n < N; ++n) {
        const float pn = __shfl(p, n, 64), wn = __shfl(W, n, 64);
        if ((lv >> n) & 1ull) { const float pw = pn * wn; risk = risk + pw; }
    }
    if (!lv) risk = __builtin_nanf("");
    float cf = 0.f;
    if (live) { const float dw = W - risk; const float pd = p * dw; cf = -(it * pd); }
    if (lane < N) {
        dist_out[slot] = d;
        post_out[slot] = p;
        coef_out[slot] = cf;
    }
    if (lane == 0) { risk_out[b] = risk; tlen_out[b] = nb; }
}

int launch_mwer_weights(const int* hyp_idx, const int* hyp_len, const float* logp, const int* status, int B, int N, int Th, const int* targets, int L,
                        const float* inv_temp, int mode, int* dist, float* post, float* risk, float* coef, int* tlen, hipStream_t s) {
    hipLaunchKernelGGL(mwer_weights_kernel, dim3((unsigned)B), dim3(64), 0, s, hyp_idx, hyp_len, logp, status, N, Th, targets, L, inv_temp, mode, dist, post,
                       risk, coef, tlen);
    return launch_rc();
}

extern "C" int ishara_mwer_weights(const int32_t* hyp_idx, const int32_t* hyp_len, const float* logp, const int32_t* status, int32_t B, int32_t N,
                                   int32_t Th, const int32_t* targets, int32_t L, const float* inv_temp, int32_t mode, int32_t* dist, float* post,
                                   float* risk, float* coef, int32_t* tlen, ishara_stream st) {
    const char* me = "ishara_mwer_weights";
    if (N < 1 || N > 64) { ishara_set_error("%s: N=%d outside 1..64 (one lane per hypothesis)", me, N); return -1; }
    if (Th < 1 || Th > 4096) { ishara_set_error("%s: Th=%d outside 1..4096", me, Th); return -1; }
    if (L < 1 || L > 64) { ishara_set_error("%s: L=%d outside 1..64 (the target is one 64-bit word)", me, L); return -1; }
    if (mode != 0 && mode != 1) { ishara_set_error("%s: mode %d is neither 0 (plain distance) nor 1 (divided by the target's length)", me, mode); return -1; }
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (B == 0) return 0;
    if (!hyp_idx || !hyp_len || !logp || !targets || !dist || !post || !risk || !coef || !tlen) {
        ishara_set_error("%s: null hyp_idx / hyp_len / logp / targets / dist / post / risk / coef / tlen (status and inv_temp may be NULL)", me); return -1;
    }
    if (((uintptr_t)hyp_idx | (uintptr_t)hyp_len | (uintptr_t)logp | (uintptr_t)status | (uintptr_t)targets | (uintptr_t)inv_temp | (uintptr_t)dist |
         (uintptr_t)post | (uintptr_t)risk | (uintptr_t)coef | (uintptr_t)tlen) % 4) {
        ishara_set_error("%s: misaligned buffer: every buffer must be 4-byte aligned", me); return -1;
    }
    return launch_mwer_weights(hyp_idx, hyp_len, logp, status, B, N, Th, targets, L, inv_temp, mode, dist, post, risk, coef, tlen, (hipStream_t)st);
}
