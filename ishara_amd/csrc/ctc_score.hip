// Exact CTC log-likelihood of every hypothesis of an n-best list under one model (ishara_ctc_score_nbest; contract in include/ishara_hip.h,
// host twin in ishara_amd/rescore.py): logp[b, n] = log sum over the alignments of hypothesis n of prod_t softmax(logits[b, t])[path_t].
//
// It is the alpha chain of ctc.hip's ctc_kernel and nothing else: no lattice in memory, no beta wave, no gradient phase, no workspace.  The
// chain's arithmetic is ctc_lattice.h's, as it is for that kernel, so logp == float32(-nll) of ishara_ctc_loss_ex bit for bit.
//
// One workgroup of CS_WAVES waves takes one clip and a group of `hpw` * CS_WAVES consecutive slots of its list:
//   phase 0 (all threads)  lse[t] = logsumexp(logits[b, t]) for t < Tn into LDS, once per workgroup
//   phase 1 (every wave)   wave w scores the slots n0 + w, n0 + w + CS_WAVES, ..: the S = 2 len + 1 lattice states in registers, state
//                          s = lane + 64 k, the s-1 / s-2 neighbours by two rotations per frame and k, emissions gathered 8 frames ahead.
//                          The extended label sequence is read from the hypothesis row itself (state s odd: symbol s >> 1), no LDS copy.
// The waves of a workgroup share nothing after the barrier behind phase 0, so a slot's result does not depend on its neighbours.
// Grid: (ceil(N / (hpw * CS_WAVES)), B).  hpw = 1 gives every hypothesis a wave of its own and recomputes lse once per four slots; a
// larger hpw shares lse among more slots and serialises their chains.  DESIGN.md §3 has the measurement that picked the default.
// LDS: lse[T] floats requested at launch (16 KiB at T = 4096), no static LDS: within the 64 KiB every launch is granted.
#include <type_traits>
#include "ctc_lattice.h"

static constexpr int CS_WAVES = 4;
static int g_cs_hpw = 0;                                // 0: the default below
extern "C" int ishara_debug_set_score_group(int32_t hyps_per_wave) { g_cs_hpw = hyps_per_wave < 0 ? 0 : (hyps_per_wave > 16 ? 16 : hyps_per_wave); return 0; }

// the alpha chain of one hypothesis by one wave; NK: compile-time count of occupied state registers (0: run-time), as in ctc_kernel.
// One arrangement differs from ctc_kernel's and changes no value: the run-time path gathers U = 4 frames ahead instead of 8.  With the
// in-place frame step it keeps the NS = 8 instantiation, the one every list in the beam search's layout at T > 127 gets, at 164 registers,
// so that the short hypotheses of such a list run at a useful occupancy.
template <int NS, int NK>
DEVI double cs_alpha(const float* __restrict__ lg, const float* __restrict__ lse, const int* __restrict__ hyp, int len, int Tn, int C, int blank,
                     int lane) {
    constexpr int U = (NK || NS <= 2) ? 8 : 4;
    const int S = 2 * len + 1;
    const int nk = NK ? NK : ((S + 63) >> 6);
    bool act[NS], skip_bw[NS];
    int my[NS];
    // the extended label sequence is read from the hypothesis row itself, no LDS copy
    ctc_states<NK>([&](int i) { return hyp[i]; }, S, blank, lane, my, act, skip_bw);
    float em[U][NS], emn[U][NS];
    double a[NS];
    ctc_alpha_init<NK>(lg, lse, len, lane, my, act, a);
    ctc_gather<NK>(lg, C, Tn, nk, my, 1, 1, emn);
    ctc_settle<NK>(lse, Tn, nk, 1, 1, emn, em);
    for (int t0 = 1; t0 < Tn; t0 += U) {
        if (t0 + U < Tn) ctc_gather<NK>(lg, C, Tn, nk, my, t0 + U, 1, emn);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (t0 + u < Tn) ctc_alpha_step_inplace<NK>(a, act, skip_bw, em[u], nk, lane);
        if (t0 + U < Tn) ctc_settle<NK>(lse, Tn, nk, t0 + U, 1, emn, em);
    }
    return ctc_alpha_final<NK>(a, S, len, lane);
}

template <int NS>
__global__ __launch_bounds__(CS_WAVES * 64) void ctc_score_kernel(const float* __restrict__ logits, int Ts, int C, int blank,
                                                                  const int* __restrict__ hyp_idx, const int* __restrict__ hyp_len, int N, int Th,
                                                                  const int* __restrict__ frame_len, int hpw, float* __restrict__ logp_out,
                                                                  int* __restrict__ status_out) {
    extern __shared__ float cs_lse[];                   // [Ts]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n0 = blockIdx.x * hpw * CS_WAVES;
    int Tn = Ts;
    if (frame_len) Tn = frame_len[b];
    if (Tn < 1 || Tn > Ts) Tn = 0;                      // no frames: never an index or a bound
    const float* lg = logits + (size_t)b * Ts * C;
    for (int t = tid; t < Tn; t += CS_WAVES * 64) cs_lse[t] = ctc_row_lse(lg + (size_t)t * C, C);
    __syncthreads();
    for (int j = 0; j < hpw; ++j) {
        const int n = n0 + j * CS_WAVES + wave;         // wave-uniform
        if (n >= N) break;
        const size_t slot = (size_t)b * N + n;
        const int len = hyp_len[slot];
        const int* hyp = hyp_idx + slot * Th;
        int st = ctc_hyp_status(hyp, len, Th, C, blank, Tn, lane);
        double lp = CTC_NEG;
        if (st == 0) {
            const int nkb = (2 * len + 1 + 63) >> 6;
            if (NS >= 2 && nkb == 1) lp = cs_alpha<NS, 1>(lg, cs_lse, hyp, len, Tn, C, blank, lane);
            else if (NS >= 3 && nkb == 2) lp = cs_alpha<NS, 2>(lg, cs_lse, hyp, len, Tn, C, blank, lane);
            else lp = cs_alpha<NS, 0>(lg, cs_lse, hyp, len, Tn, C, blank, lane);
            if (!(lp > -1e29)) st = CTC_HYP_NOALIGN;
        }
        if (lane == 0) {
            logp_out[slot] = st ? -INFINITY : -(float)(-lp);      // the loss writes (float)(-logp)
            if (status_out) status_out[slot] = st;
        }
    }
}

extern "C" int ishara_ctc_score_nbest(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, const int32_t* hyp_idx,
                                      const int32_t* hyp_len, int32_t N, int32_t Th, const int32_t* frame_len, float* logp, int32_t* status,
                                      ishara_stream st) {
    const char* me = "ishara_ctc_score_nbest";
    if (C < 2 || C > 64) { ishara_set_error("%s: C=%d outside 2..64", me, C); return -1; }
    if (T < 1 || T > 4096) { ishara_set_error("%s: T=%d outside 1..4096", me, T); return -1; }
    if (Th < 1 || Th > 4096) { ishara_set_error("%s: Th=%d outside 1..4096 (the width of the hypothesis rows)", me, Th); return -1; }
    if (N < 1 || N > 64) { ishara_set_error("%s: N=%d outside 1..64", me, N); return -1; }
    if (blank < 0 || blank >= C) { ishara_set_error("%s: blank %d outside 0..%d", me, blank, C - 1); return -1; }
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (B > 65535) { ishara_set_error("%s: B=%d > 65535 (one grid row per clip)", me, B); return -1; }
    if (B == 0) return 0;
    if (!logits || !hyp_idx || !hyp_len || !logp) { ishara_set_error("%s: null logits / hyp_idx / hyp_len / logp (frame_len and status may be NULL)", me); return -1; }
    if (((uintptr_t)logits | (uintptr_t)hyp_idx | (uintptr_t)hyp_len | (uintptr_t)frame_len | (uintptr_t)logp | (uintptr_t)status) % 4) {
        ishara_set_error("%s: misaligned buffer: every buffer must be 4-byte aligned", me); return -1;
    }
    const int lmax = Th < 255 ? Th : 255, ns = (2 * lmax + 1 + 63) / 64;
    // Every hypothesis a wave of its own while the device holds all B * N waves at once: 256 CUs x 4 SIMDs x the instantiation's occupancy
    // (7 / 5 / 4 / 3 waves per SIMD at NS = 1 / 2 / 4 / 8).  Beyond that a wave takes ceil(B N / resident) slots one after the other and
    // the clip's lse is computed for fewer workgroups.  Measured at B 64, T 384 (profiles/r23_nbest_rescore.json): one slot per wave wins
    // at N <= 32 (2048 waves), two per wave at N 64 (4096 waves against 3072 resident); four per wave leaves SIMDs empty and loses at every N.
    int hpw = g_cs_hpw;
    if (hpw == 0) {
        const long long resident = 1024LL * (ns <= 1 ? 7 : ns <= 2 ? 5 : ns <= 4 ? 4 : 3);
        const long long want = ((long long)B * N + resident - 1) / resident;
        hpw = (int)(want < 1 ? 1 : (want > 16 ? 16 : want));
    }
    const int per = hpw * CS_WAVES;
    const dim3 grid((unsigned)((N + per - 1) / per), (unsigned)B), block(CS_WAVES * 64);
    const size_t shmem = (size_t)T * sizeof(float);
#define CS_LAUNCH(NSV) hipLaunchKernelGGL((ctc_score_kernel<NSV>), grid, block, shmem, (hipStream_t)st, logits, T, C, blank, hyp_idx, hyp_len, N, Th, frame_len, hpw, logp, status)
    if (ns <= 1) CS_LAUNCH(1);
    else if (ns <= 2) CS_LAUNCH(2);
    else if (ns <= 4) CS_LAUNCH(4);
    else CS_LAUNCH(8);
#undef CS_LAUNCH
    return launch_rc();
}
