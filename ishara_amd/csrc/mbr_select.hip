// Minimum-Bayes-risk selection over an n-best list (ishara_mbr_select; contract in include/ishara_hip.h, host twin in ishara_amd/mbr.py):
// per clip the hypothesis with the smallest expected edit distance to the others, the others voting with exp((score - max) / temperature)
// or with explicit weights.
//
// One workgroup of MB_WAVES waves per clip, one kernel, no workspace.
//   1. stage    wave w takes the hypotheses w, w + MB_WAVES, ...: lane k loads symbol k (k < min(len, T, 64), nothing else is read), checks it
//               against [0, C), stores it as a byte and, by one ballot per class, builds the match masks peq[n][c] (bit k: symbol k is c).
//   2. pairs    the N (N - 1) / 2 pairs i < j are spread over the lanes (the strict upper triangle folded into N / 2 rows of N, so that no
//               lane idles on the lower half): edit_distance.h's myers (Hyyro's bit-vector form), pattern i in one 64-bit word, len_j steps of
//               integer operations, global (not substring) distance.  d goes to LDS as a byte, both halves.
//   3. votes    wave 0, lane = slot: the maximum over the finite scores by the xor butterfly (a maximum does not depend on its tree),
//               x = (s - max) * inv_temp in two roundings, expf.
//   4. risk     lane i sums w_j * c_ij over the live j in ascending order, every operation rounded on its own (fp contraction off), then
//               every lane of the wave walks the risks in slot order by readlane and keeps the first strict minimum.
//   5. copy     all lanes copy the selected row and write dist.
// LDS: peq 64 x 64 x 8 = 32 KB, symbols and distances 4 KB each as bytes, under 41 KB in all (static; three clips per CU).  A clip with a
// hypothesis longer than 64 symbols or a symbol outside [0, C) is not ranked (status, contract); such a symbol never becomes an index.
// Integer distances, fixed summation order, no atomics: bit-identical from run to run.
#include "edit_distance.h"

static constexpr int MB_WAVES = 4;
static constexpr int MB_MAXN = 64;
static constexpr int MB_MAXL = 64;                      // MAX_PHRASE_LENGTH: one 64-bit word per pattern

// r + w * c, c = d or d / max(len_j, 1): the division, the multiplication and the addition each rounded on its own.  hipcc contracts
// a * b + c into an FMA by default, and __fmul_rn / __fadd_rn are plain operators in its headers that carry the same permission into the
// caller once inlined, so the operators are written out under the pragma (as awp.hip's awp_step and weight_avg.hip's wavg_blend do).
DEVI float mb_x(float s, float smax, float it) {
#pragma clang fp contract(off)
    const float d = s - smax;
    return d * it;
}
DEVI float mb_acc(float r, float w, int d, int len_j, int mode) {
#pragma clang fp contract(off)
    float c = (float)d;
    if (mode == 1) c = c / (float)(len_j > 1 ? len_j : 1);
    const float p = w * c;
    return r + p;
}

__global__ __launch_bounds__(MB_WAVES * 64) void mbr_select_kernel(const int* __restrict__ hyp_idx, const int* __restrict__ hyp_len,
                                                                   const float* __restrict__ hyp_score, const float* __restrict__ weights,
                                                                   const float* __restrict__ inv_temp, int N, int T, int C, int mode,
                                                                   int* __restrict__ out_idx, int* __restrict__ out_len, int* __restrict__ best_out,
                                                                   float* __restrict__ risk_out, float* __restrict__ w_out, int* __restrict__ dist_out,
                                                                   int* __restrict__ status_out) {
    __shared__ uint64_t s_peq[MB_MAXN][64];
    __shared__ uint8_t s_sym[MB_MAXN][MB_MAXL];
    __shared__ uint8_t s_dist[MB_MAXN][MB_MAXN];
    __shared__ int s_len[MB_MAXN];                      // clamped to T; -1: dead
    __shared__ int s_best;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* __restrict__ hyp = hyp_idx + (size_t)b * N * T;
    const int* __restrict__ lens = hyp_len + (size_t)b * N;

    // ---- 1. lengths, symbols, match masks
    int flags = 0;                                      // bit 0: a live hypothesis longer than 64; bit 1: a live symbol outside [0, C)
    for (int n = wave; n < N; n += MB_WAVES) {          // uniform per wave
        int len = lens[n];
        len = len < 0 ? -1 : (len > T ? T : len);
        if (lane == 0) s_len[n] = len;
        if (len > MB_MAXL) flags |= 1;
        const int take = len < 0 ? 0 : (len > MB_MAXL ? MB_MAXL : len);
        const bool have = lane < take;
        const int sym = have ? hyp[(size_t)n * T + lane] : -1;
        const bool ok = have && sym >= 0 && sym < C;
        if (have && !ok) flags |= 2;
        s_sym[n][lane] = ok ? (uint8_t)sym : 0;
        uint64_t mine = 0;
        for (int c = 0; c < C; ++c) {
            const uint64_t m = __ballot(ok && sym == c);
            if (lane == c) mine = m;
        }
        s_peq[n][lane] = mine;                          // lanes >= C: 0, never read (text bytes are < C)
    }
    const int st_long = __syncthreads_or(flags & 1);    // also the barrier behind the staging
    const int st_bad = __syncthreads_or(flags & 2);
    const bool ranked = !st_long && !st_bad;

    // ---- 2. pairwise distances
    if (ranked) {
        const int rows = N >> 1, items = rows * N;
        for (int q = tid; q < items; q += MB_WAVES * 64) {
            const int r = q / N, c = q - r * N;
            int i, j;
            if (c < N - 1 - r) { i = r; j = r + 1 + c; }
            else { i = N - 2 - r; j = i + 1 + (c - (N - 1 - r)); if (i == r) continue; }      // the middle row of an odd triangle folds onto itself
            const int li = s_len[i], lj = s_len[j];
            if (li < 0 || lj < 0) continue;
            const uint64_t* peq = s_peq[i];
            const uint8_t* text = s_sym[j];             // bytes < C <= 64: every symbol has its row of the table
            const int d = myers(li, [&](int k) { return peq[text[k]]; }, lj);
            s_dist[i][j] = (uint8_t)d;
            s_dist[j][i] = (uint8_t)d;
        }
        if (tid < N) s_dist[tid][tid] = 0;
    }
    __syncthreads();

    // ---- 3. votes, 4. risk and selection: wave 0, lane = slot
    if (wave == 0) {
        const int len = lane < N ? s_len[lane] : -1;
        const bool live = len >= 0;
        float w = 0.f;
        if (weights) {
            const float v = live ? weights[(size_t)b * N + lane] : 0.f;
            w = (v > 0.f && v < INFINITY) ? v : 0.f;    // NaN fails both comparisons
        } else {
            const float s = live ? hyp_score[(size_t)b * N + lane] : -INFINITY;
            const bool fin = fabsf(s) < INFINITY;       // false for NaN
            const float smax = wave_max(fin ? s : -INFINITY);
            const float it = inv_temp ? inv_temp[0] : 1.f;
            if (fin) w = expf(mb_x(s, smax, it));
        }
        if (w_out && lane < N) w_out[(size_t)b * N + lane] = w;
        const unsigned long long alive = __ballot(live);
        const int first = alive ? (int)__builtin_ctzll(alive) : -1;
        float risk = 0.f;
        if (ranked) {
            for (int j = 0; j < N; ++j) {               // uniform: the whole wave walks the voters, dead lanes sum what nobody reads
                const int lj = s_len[j];
                const float wj = __shfl(w, j);
                if (lj < 0) continue;
                risk = mb_acc(risk, wj, live ? (int)s_dist[lane][j] : 0, lj, mode);
            }
        }
        if (!ranked || !live) risk = __uint_as_float(0x7fc00000u);      // dead slots and unranked clips: NaN
        if (risk_out && lane < N) risk_out[(size_t)b * N + lane] = risk;
        int best = first;
        if (ranked && first >= 0) {
            float rb = __shfl(risk, first);
            for (int i = first + 1; i < N; ++i) {       // uniform: every lane follows the same walk
                const float ri = __shfl(risk, i);
                if (((alive >> i) & 1ull) && ri < rb) { rb = ri; best = i; }
            }
        }
        if (lane == 0) {
            s_best = best;
            best_out[b] = best;
            out_len[b] = best >= 0 ? s_len[best] : 0;
            if (status_out) status_out[b] = (st_long ? 1 : 0) | (st_bad ? 2 : 0) | (first < 0 ? 4 : 0);
        }
    }
    __syncthreads();

    // ---- 5. the selected row in the greedy layout, and dist
    const int best = s_best;
    const int blen = best >= 0 ? s_len[best] : 0;
    for (int t = tid; t < T; t += MB_WAVES * 64) out_idx[(size_t)b * T + t] = t < blen ? hyp[(size_t)best * T + t] : -1;
    if (dist_out) {
        for (int q = tid; q < N * N; q += MB_WAVES * 64) {
            const int i = q / N, j = q - i * N;
            dist_out[(size_t)b * N * N + q] = (ranked && s_len[i] >= 0 && s_len[j] >= 0) ? (int)s_dist[i][j] : -1;
        }
    }
}

extern "C" int ishara_mbr_select(const int32_t* hyp_idx, const int32_t* hyp_len, const float* hyp_score, const float* weights, const float* inv_temp,
                                 int32_t B, int32_t N, int32_t T, int32_t C, int32_t mode, int32_t* out_idx, int32_t* out_len, int32_t* best,
                                 float* risk, float* w_out, int32_t* dist, int32_t* status, ishara_stream st) {
    const char* me = "ishara_mbr_select";
    if (N < 1 || N > MB_MAXN) { ishara_set_error("%s: N=%d outside 1..%d (one lane per hypothesis)", me, N, MB_MAXN); return -1; }
    if (T < 1 || T > 4096) { ishara_set_error("%s: T=%d outside 1..4096", me, T); return -1; }
    if (C < 2 || C > 64) { ishara_set_error("%s: C=%d outside 2..64 (one lane per class)", me, C); return -1; }
    if (mode != 0 && mode != 1) { ishara_set_error("%s: unknown mode %d (0 edit distance, 1 normalised by the voter's length)", me, mode); return -1; }
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (B == 0) return 0;
    if (!hyp_idx || !hyp_len) { ishara_set_error("%s: null hyp_idx / hyp_len", me); return -1; }
    if (!hyp_score && !weights) { ishara_set_error("%s: null hyp_score without weights: nothing to vote with", me); return -1; }
    if (!out_idx || !out_len || !best) { ishara_set_error("%s: null out_idx / out_len / best", me); return -1; }
    const uintptr_t bits = (uintptr_t)hyp_idx | (uintptr_t)hyp_len | (uintptr_t)hyp_score | (uintptr_t)weights | (uintptr_t)inv_temp | (uintptr_t)out_idx |
                           (uintptr_t)out_len | (uintptr_t)best | (uintptr_t)risk | (uintptr_t)w_out | (uintptr_t)dist | (uintptr_t)status;
    if (bits % 4) { ishara_set_error("%s: misaligned buffer: every buffer must be 4-byte aligned", me); return -1; }
    if (bytes_overlap(out_idx, (size_t)B * T * 4, hyp_idx, (size_t)B * N * T * 4)) { ishara_set_error("%s: out_idx overlaps hyp_idx", me); return -1; }
    hipLaunchKernelGGL(mbr_select_kernel, dim3((unsigned)B), dim3(MB_WAVES * 64), 0, (hipStream_t)st, hyp_idx, hyp_len, hyp_score, weights, inv_temp,
                       N, T, C, mode, out_idx, out_len, best, risk, w_out, dist, status);
    return launch_rc();
}
