// The weight sweep of n-best rescoring (ishara_rescore_sweep; contract in include/ishara_hip.h, host twin rescore_sweep_reference in
// ishara_amd/rescore.py): for every row g of a grid of rescoring parameters (w_0 .. w_{M-1}, alpha, beta) the slot that tops each clip's
// list under that row and its edit distance to the clip's target, i.e. G x (ishara_nbest_rescore_p + ishara_edit_distance) in one launch.
//
// Nothing but the argmax depends on the row, so a workgroup (RS_WAVES waves) owns one clip and RS_ROWS consecutive rows and computes the
// clip's part once, into LDS:
//   1. stage    all threads copy the workgroup's rows of the grid into LDS (the loads fly during 2 and 3); wave 0, lane = slot: the
//               lengths clamped to Th; wave 1, lane = target position: the target, its length (symbols before the first 59) and the match
//               masks peq[c] (bit j: target symbol j is c) by one ballot per class.
//   2. dedupe   nbest_rescore.hip's: the pairs i < j over the threads, an equal pair of live slots marks j.
//   3. walks    wave 0, lane = slot: the LM automaton walk l (float32, in order) of every slot that is live on input; wave 1, lane = slot:
//               the slot's distance to the target by Hyyro's bit-vector form of Myers' algorithm with the TARGET as the pattern (<= 64
//               symbols: one 64-bit word, edit_distance.h's myers) and the hypothesis as the text, any length up to Th; with fallback
//               the text of a hypothesis shorter than 3 is the constant phrase; one lane of wave 2: the constant phrase's own distance.
//   4. rows     every wave takes the rows wave, wave + RS_WAVES, ...; lane = slot holds live / len / l / the M scores in registers:
//               the score in nbest_rescore.hip's order (M + 2 rounded multiply-adds, contraction off), the maximum over the slots whose
//               score is a number by the xor butterfly (a maximum does not depend on its tree), one ballot of the lanes that hold it: the
//               lowest set bit is the tie rule.  No number: the first live slot (a NaN); no live slot: -1.  Lane 0 stores two integers.
// The per-clip part is recomputed by each of a clip's ceil(G / RS_ROWS) workgroups rather than handed over through a workspace by a
// kernel of its own: it costs less than a second launch, and at G <= RS_ROWS nothing is recomputed.  So the
// workspace is 0 bytes.  Integer distances, float32 operations in a fixed order, no atomics: bit-identical from run to run.
#include "rescore_common.h"
#include "edit_distance.h"

static constexpr int RS_WAVES = 4;
static constexpr int RS_ROWS = 256;                     // grid rows per workgroup; mirrored as SWEEP_ROW_TILE in ishara_amd/rescore.py
static constexpr int RS_MAXL = 64;                      // MAX_PHRASE_LENGTH: the target is one 64-bit word

__global__ __launch_bounds__(RS_WAVES * 64) void rescore_sweep_kernel(const int* __restrict__ hyp_idx, const int* __restrict__ hyp_len, int B, int N, int Th,
                                                                      NrPtrs logp, int M, const float* __restrict__ lm_logp, const int* __restrict__ lm_next,
                                                                      int S, int start_state, int C, int blank, const int* __restrict__ targets, int L,
                                                                      int fallback, const float* __restrict__ grid, int G, int* __restrict__ best_out,
                                                                      int* __restrict__ dist_out, int* __restrict__ tlen_out, int* __restrict__ hyp_dist,
                                                                      float* __restrict__ lm_score) {
    __shared__ float s_grid[RS_ROWS * (NR_MAX_M + 2)];
    __shared__ uint64_t s_peq[64];
    __shared__ int s_tgt[RS_MAXL];
    __shared__ int s_len[NR_MAXN];                      // clamped to Th; -1: dead on input
    __shared__ int s_dup[NR_MAXN];
    __shared__ int s_hd[NR_MAXN];                       // distance to the target of a slot that is live on input (after the fallback rule)
    __shared__ float s_l[NR_MAXN];
    __shared__ int s_bad[NR_MAXN];                      // a symbol outside [0, C): the score is -inf
    __shared__ int s_nb, s_dfb;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = blockIdx.y * RS_ROWS;
    const int rows = G - g0 < RS_ROWS ? G - g0 : RS_ROWS;
    const int P = M + 2;
    const int* __restrict__ hyp = hyp_idx + (size_t)b * N * Th;

    // ---- 1. the rows of the grid, lengths, the target
    for (int q = tid; q < rows * P; q += RS_WAVES * 64) s_grid[q] = grid[(size_t)g0 * P + q];
    if (wave == 0) {
        int len = lane < N ? hyp_len[(size_t)b * N + lane] : -1;
        len = len < 0 ? -1 : (len > Th ? Th : len);
        s_len[lane] = len;
        s_dup[lane] = 0;
    } else if (wave == 1) {
        const int nb = target_prep(targets + (size_t)b * L, L, lane, s_tgt, s_peq);
        if (lane == 0) s_nb = nb;
    }
    __syncthreads();

    // ---- 2. duplicates: j dies when a live i < j holds the same string
    for (int q = tid; q < N * N; q += RS_WAVES * 64) {
        const int i = q / N, j = q - i * N;
        if (i >= j) continue;
        const int li = s_len[i], lj = s_len[j];
        if (li < 0 || li != lj) continue;
        bool same = true;
        for (int k = 0; k < li && same; ++k) same = hyp[(size_t)i * Th + k] == hyp[(size_t)j * Th + k];
        if (same) s_dup[j] = 1;
    }

    // ---- 3. the walks that do not depend on the merge
    if (wave == 0) {
        const int len = s_len[lane];
        float l = 0.f;
        bool bad = false;
        if (lm_logp && len >= 0) {
            int state = start_state;
            for (int k = 0; k < len; ++k) {
                const int c = hyp[(size_t)lane * Th + k];
                if (c < 0 || c >= C) { bad = true; break; }                           // never an index
                l = l + lm_logp[(size_t)state * C + c];
                const int nx = lm_next[(size_t)state * C + c];
                state = (nx >= 0 && nx < S) ? nx : 0;
            }
            if (!bad) l = l + lm_logp[(size_t)state * C + blank];
        }
        s_l[lane] = l;
        s_bad[lane] = bad ? 1 : 0;
    } else if (wave == 1) {
        const int len = s_len[lane], nb = s_nb;
        int d = -1;
        if (len >= 0) {
            const bool fb = fallback && len < 3;
            const int* text = fb ? fallback_phrase : hyp + (size_t)lane * Th;
            d = myers(nb, [&](int k) { return match_mask(s_peq, s_tgt, nb, text[k]); }, fb ? FALLBACK_LEN : len);
        }
        s_hd[lane] = d;
    } else if (tid == 2 * 64) {
        const int nb = s_nb;
        s_dfb = myers(nb, [&](int k) { return match_mask(s_peq, s_tgt, nb, fallback_phrase[k]); }, FALLBACK_LEN);
    }
    __syncthreads();

    // ---- 4. the rows: lane = slot
    const int len = (lane < N && !s_dup[lane]) ? s_len[lane] : -1;
    const bool live = len >= 0;
    const float l = live ? s_l[lane] : 0.f;
    const bool bad = live && s_bad[lane];
    const float flen = (float)len;
    const int nb = s_nb;
    const int none_d = fallback ? s_dfb : nb;           // no live slot: the constant phrase, or the empty string
    float lp[NR_MAX_M];
#pragma unroll
    for (int m = 0; m < NR_MAX_M; ++m) lp[m] = (m < M && live) ? logp.p[m][(size_t)b * N + lane] : 0.f;
    const unsigned long long alive = __ballot(live);
    const int first_live = alive ? (int)__builtin_ctzll(alive) : -1;

    if (blockIdx.y == 0 && wave == 0) {                 // the outputs that no row changes
        if (lane == 0) tlen_out[b] = nb;
        if (lane < N) {
            if (hyp_dist) hyp_dist[(size_t)b * N + lane] = live ? s_hd[lane] : -1;
            if (lm_score) lm_score[(size_t)b * N + lane] = live ? (bad ? -INFINITY : l) : 0.f;
        }
    }

    for (int r = wave; r < rows; r += RS_WAVES) {       // uniform per wave
        const float* __restrict__ p = s_grid + r * P;
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < NR_MAX_M; ++m) {
            if (m >= M) break;
            const float w = p[m];
            if (w > 0.f) s = nr_madd(s, w, lp[m]);      // a weight that is not > 0 (NaN too): the model takes no part
        }
        if (lm_logp) s = bad ? -INFINITY : nr_madd(s, p[M], l);
        s = nr_madd(s, p[M + 1], flen);
        const bool num = live && s == s;
        int win = first_live;                           // no number: the first live slot holds the first live NaN
        if (__ballot(num)) {
            const float smax = wave_max(num ? s : -INFINITY);
            win = (int)__builtin_ctzll(__ballot(num && s == smax));      // -inf is a number: s == smax holds for it when nothing is larger
        }
        if (lane == 0) {
            const size_t o = (size_t)(g0 + r) * B + b;
            best_out[o] = win;
            dist_out[o] = win >= 0 ? s_hd[win] : none_d;
        }
    }
}

extern "C" int64_t ishara_rescore_sweep_workspace_bytes(int32_t B, int32_t N, int32_t G) {
    if (B < 0 || N < 1 || N > NR_MAXN || G < 1 || G > 65536) return -1;
    return 0;
}

extern "C" int ishara_rescore_sweep(const int32_t* hyp_idx, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Th, const float* const* logp, int32_t M,
                                    const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state, int32_t C, int32_t blank,
                                    const int32_t* targets, int32_t L, int32_t fallback, const float* grid, int32_t G, int32_t* best, int32_t* dist,
                                    int32_t* tlen, int32_t* hyp_dist, float* lm_score, void* ws, ishara_stream st) {
    const char* me = "ishara_rescore_sweep";
    (void)ws;                                           // ishara_rescore_sweep_workspace_bytes is 0: never looked at
    if (N < 1 || N > NR_MAXN) { ishara_set_error("%s: N=%d outside 1..%d (one lane per hypothesis)", me, N, NR_MAXN); return -1; }
    if (Th < 1 || Th > 4096) { ishara_set_error("%s: Th=%d outside 1..4096", me, Th); return -1; }
    if (M < 1 || M > NR_MAX_M) { ishara_set_error("%s: M=%d outside 1..%d (the models' pointers travel in the kernel's arguments)", me, M, NR_MAX_M); return -1; }
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (G < 1 || G > 65536) { ishara_set_error("%s: G=%d grid rows outside 1..65536", me, G); return -1; }
    if (L < 1 || L > RS_MAXL) { ishara_set_error("%s: target length L=%d unsupported (1..%d: the target is one 64-bit word)", me, L, RS_MAXL); return -1; }
    if (fallback != 0 && fallback != 1) { ishara_set_error("%s: fallback %d is neither 0 (score the hypothesis as it is) nor 1 (the wrapper's rule)", me, fallback); return -1; }
    const bool with_lm = lm_logp || lm_next;
    if (with_lm) {
        if (C < 2 || C > 64) { ishara_set_error("%s: C=%d outside 2..64", me, C); return -1; }
        if (blank < 0 || blank >= C) { ishara_set_error("%s: blank %d outside 0..%d", me, blank, C - 1); return -1; }
        if (S < 1 || S > (1 << 22)) { ishara_set_error("%s: S=%d states unsupported (1..2^22)", me, S); return -1; }
        if (start_state < 0 || start_state >= S) { ishara_set_error("%s: start_state %d outside 0..%d", me, start_state, S - 1); return -1; }
        if (!lm_logp || !lm_next) { ishara_set_error("%s: lm_logp and lm_next go together: both NULL (no LM) or both given", me); return -1; }
        if (((uintptr_t)lm_logp | (uintptr_t)lm_next) % 16) { ishara_set_error("%s: lm_logp and lm_next must be 16-byte aligned", me); return -1; }
    }
    if (B == 0) return 0;
    if (!hyp_idx || !hyp_len) { ishara_set_error("%s: null hyp_idx / hyp_len", me); return -1; }
    if (!logp) { ishara_set_error("%s: null logp", me); return -1; }
    for (int m = 0; m < M; ++m)
        if (!logp[m]) { ishara_set_error("%s: null logp[%d]", me, m); return -1; }
    if (!targets || !grid) { ishara_set_error("%s: null targets / grid", me); return -1; }
    if (!best || !dist || !tlen) { ishara_set_error("%s: null best / dist / tlen (hyp_dist and lm_score may be NULL)", me); return -1; }
    uintptr_t bits = (uintptr_t)hyp_idx | (uintptr_t)hyp_len | (uintptr_t)targets | (uintptr_t)grid | (uintptr_t)best | (uintptr_t)dist | (uintptr_t)tlen |
                     (uintptr_t)hyp_dist | (uintptr_t)lm_score;
    for (int m = 0; m < M; ++m) bits |= (uintptr_t)logp[m];
    if (bits % 4) { ishara_set_error("%s: misaligned buffer: every buffer must be 4-byte aligned", me); return -1; }
    const size_t bn = (size_t)B * N * 4, bnt = bn * Th, gb = (size_t)G * B * 4;
    const void* outs[5] = {best, dist, tlen, hyp_dist, lm_score};
    const size_t osz[5] = {gb, gb, (size_t)B * 4, bn, bn};
    const char* onm[5] = {"best", "dist", "tlen", "hyp_dist", "lm_score"};
    for (int o = 0; o < 5; ++o) {
        if (bytes_overlap(outs[o], osz[o], hyp_idx, bnt)) { ishara_set_error("%s: %s overlaps hyp_idx", me, onm[o]); return -1; }
        if (bytes_overlap(outs[o], osz[o], hyp_len, bn)) { ishara_set_error("%s: %s overlaps hyp_len", me, onm[o]); return -1; }
        if (bytes_overlap(outs[o], osz[o], targets, (size_t)B * L * 4)) { ishara_set_error("%s: %s overlaps targets", me, onm[o]); return -1; }
        if (bytes_overlap(outs[o], osz[o], grid, (size_t)G * (M + 2) * 4)) { ishara_set_error("%s: %s overlaps grid", me, onm[o]); return -1; }
        for (int m = 0; m < M; ++m)
            if (bytes_overlap(outs[o], osz[o], logp[m], bn)) { ishara_set_error("%s: %s overlaps logp[%d]", me, onm[o], m); return -1; }
    }
    NrPtrs in;
    for (int m = 0; m < NR_MAX_M; ++m) in.p[m] = m < M ? logp[m] : nullptr;
    hipLaunchKernelGGL(rescore_sweep_kernel, dim3((unsigned)B, (unsigned)((G + RS_ROWS - 1) / RS_ROWS)), dim3(RS_WAVES * 64), 0, (hipStream_t)st, hyp_idx,
                       hyp_len, B, N, Th, in, M, lm_logp, lm_next, S, start_state, C, blank, targets, L, fallback, grid, G, best, dist, tlen, hyp_dist,
                       lm_score);
    return launch_rc();
}
