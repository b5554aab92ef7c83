// Second-pass n-best rescoring (ishara_nbest_rescore; contract in include/ishara_hip.h, host twin in ishara_amd/rescore.py): per clip the
// scores of M models and an optional LM automaton combined per hypothesis, duplicate strings merged into their first slot, the list
// reordered by the new score, and a posterior over it.
//
// One workgroup of NR_WAVES waves per clip, one kernel, no workspace, no atomics.
//   1. lengths  lane = slot (wave 0 of the loads, every thread of the LDS copy): live iff hyp_len >= 0, the length clamped to Th.
//   2. dedupe   the N (N - 1) / 2 pairs i < j spread over the threads; a pair of live slots of equal length is compared symbol by symbol and
//               an equal pair marks j (a plain LDS store of 1: every writer writes the same value).
//   3. score    wave 0, lane = slot: the M weighted model scores in ascending m, the LM walk (a chain of dependent table reads per lane),
//               the length bonus; every operation rounded on its own (fp contraction off).
//   4. order    rank of a slot = the number of slots that precede it, counted by one rotation over the wave: live numbers by descending
//               score (ties to the lower slot), then live NaNs, then the dead, each in input order.  perm[rank] = slot through LDS.
//   5. posterior lane = output slot: max over the finite scores by the xor butterfly, x = (s - max) * inv_temp in two roundings, expf, the
//               sum walked in ascending output order by every lane alike, one division.
//   6. copy     all threads copy the rows in the new order; every element of every output is written.
// The M model pointers travel in the kernel's arguments (logits_combine.hip's idiom); weights and inv_temp are read on the device at every
// launch, so a captured graph follows a caller that rewrites them.  ishara_nbest_rescore_p is the same kernel with alpha and beta read from
// the device as well: params = (w_0 .. w_{M-1}, alpha, beta); the kernel's `weights` then points at params and `ab` behind the weights.
#include "rescore_common.h"

static constexpr int NR_WAVES = 4;

DEVI float nr_x(float s, float smax, float it) {
#pragma clang fp contract(off)
    const float d = s - smax;
    return d * it;
}

__global__ __launch_bounds__(NR_WAVES * 64) void nbest_rescore_kernel(const int* __restrict__ hyp_idx, const int* __restrict__ hyp_len, int N, int Th,
                                                                      NrPtrs logp, int M, const float* __restrict__ weights,
                                                                      const float* __restrict__ lm_logp, const int* __restrict__ lm_next, int S,
                                                                      int start_state, int C, int blank, float alpha, float beta,
                                                                      const float* __restrict__ ab, const float* __restrict__ inv_temp, int* __restrict__ out_idx,
                                                                      int* __restrict__ out_len, float* __restrict__ out_score,
                                                                      float* __restrict__ posterior, int* __restrict__ perm_out) {
    __shared__ int s_len[NR_MAXN];                      // clamped to Th; -1: dead (on input, or a duplicate after step 2)
    __shared__ int s_dup[NR_MAXN];
    __shared__ int s_perm[NR_MAXN];
    __shared__ int s_olen[NR_MAXN];                     // the output slots' lengths
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int* __restrict__ hyp = hyp_idx + (size_t)b * N * Th;
    if (ab) { alpha = ab[0]; beta = ab[1]; }            // the _p entry: the two numbers of this launch, read like the weights

    // ---- 1. lengths
    if (tid < NR_MAXN) {
        int len = tid < N ? hyp_len[(size_t)b * N + tid] : -1;
        len = len < 0 ? -1 : (len > Th ? Th : len);
        s_len[tid] = len;
        s_dup[tid] = 0;
    }
    __syncthreads();

    // ---- 2. duplicates: j dies when a live i < j holds the same string
    for (int q = tid; q < N * N; q += NR_WAVES * 64) {
        const int i = q / N, j = q - i * N;
        if (i >= j) continue;
        const int li = s_len[i], lj = s_len[j];
        if (li < 0 || li != lj) continue;
        bool same = true;
        for (int k = 0; k < li && same; ++k) same = hyp[(size_t)i * Th + k] == hyp[(size_t)j * Th + k];
        if (same) s_dup[j] = 1;
    }
    __syncthreads();

    // ---- 3. score, 4. order, 5. posterior: wave 0
    if (wave == 0) {
        const int len = (lane < N && !s_dup[lane]) ? s_len[lane] : -1;
        const bool live = len >= 0;
        float s = 0.f;
        if (live) {
#pragma unroll
            for (int m = 0; m < NR_MAX_M; ++m) {
                if (m >= M) break;
                const float w = weights[m];
                if (w > 0.f) s = nr_madd(s, w, logp.p[m][(size_t)b * N + lane]);      // a weight that is not > 0 (NaN too): the model is not read
            }
            if (lm_logp) {
                float l = 0.f;
                int state = start_state;
                bool bad = false;
                for (int k = 0; k < len; ++k) {
                    const int c = hyp[(size_t)lane * Th + k];
                    if (c < 0 || c >= C) { bad = true; break; }                       // never an index
                    l = l + lm_logp[(size_t)state * C + c];
                    const int nx = lm_next[(size_t)state * C + c];
                    state = (nx >= 0 && nx < S) ? nx : 0;
                }
                if (bad) s = -INFINITY;
                else {
                    l = l + lm_logp[(size_t)state * C + blank];
                    s = nr_madd(s, alpha, l);
                }
            }
            s = nr_madd(s, beta, (float)len);
        }
        // class 0: a live number, 1: a live NaN, 2: dead
        const int cls = !live ? 2 : (s != s ? 1 : 0);
        int rank = 0;
        for (int j = 0; j < N; ++j) {                   // uniform
            const float sj = __shfl(s, j);
            const int cj = __shfl(cls, j);
            const bool before = cj < cls || (cj == cls && (cls == 0 ? (sj > s || (sj == s && j < lane)) : j < lane));
            rank += (j != lane && before) ? 1 : 0;
        }
        if (lane < N) s_perm[rank] = lane;
        // lane = output slot from here on (LDS written and read by this wave alone; the fence orders the two)
        __threadfence_block();
        const int src = lane < N ? s_perm[lane] : 0;
        const float so = __shfl(s, src);
        const int lo = __shfl(len, src);
        const bool live_o = lane < N && lo >= 0;
        const bool fin = live_o && fabsf(so) < INFINITY;                              // false for NaN
        const float smax = wave_max(fin ? so : -INFINITY);
        const float it = inv_temp ? inv_temp[0] : 1.f;
        const float e = fin ? expf(nr_x(so, smax, it)) : 0.f;
        float sum = 0.f;
        for (int r = 0; r < N; ++r) sum = sum + __shfl(e, r);                          // ascending output order from +0
        if (lane < N) {
            const size_t o = (size_t)b * N + lane;
            out_len[o] = live_o ? lo : -1;
            out_score[o] = live_o ? so : -INFINITY;
            if (posterior) posterior[o] = (fin && sum > 0.f) ? e / sum : 0.f;
            if (perm_out) perm_out[o] = src;
            s_olen[lane] = live_o ? lo : -1;
        }
    }
    __syncthreads();

    // ---- 6. the rows in the new order
    for (int r = wave; r < N; r += NR_WAVES) {
        const int src = s_perm[r], len = s_olen[r];
        int* __restrict__ o = out_idx + ((size_t)b * N + r) * Th;
        for (int t = lane; t < Th; t += 64) o[t] = t < len ? hyp[(size_t)src * Th + t] : -1;
    }
}

// both entries: `params` NULL is the by-value entry (weights, alpha, beta), otherwise weights / alpha / beta are not looked at
static int nr_run(const char* me, const int32_t* hyp_idx, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Th, const float* const* logp, int32_t M,
                  const float* weights, const float* params, const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state, int32_t C,
                  int32_t blank, float alpha, float beta, const float* inv_temp, int32_t* out_idx, int32_t* out_len, float* out_score, float* posterior,
                  int32_t* perm, ishara_stream st, bool by_value) {
    if (N < 1 || N > NR_MAXN) { ishara_set_error("%s: N=%d outside 1..%d (one lane per hypothesis)", me, N, NR_MAXN); return -1; }
    if (Th < 1 || Th > 4096) { ishara_set_error("%s: Th=%d outside 1..4096", me, Th); return -1; }
    if (M < 1 || M > NR_MAX_M) { ishara_set_error("%s: M=%d outside 1..%d (the models' pointers travel in the kernel's arguments)", me, M, NR_MAX_M); return -1; }
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (by_value && (!(alpha == alpha && beta == beta) || alpha - alpha != 0.0f || beta - beta != 0.0f)) { ishara_set_error("%s: alpha and beta must be finite", me); return -1; }
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
    if (by_value && !weights) { ishara_set_error("%s: null weights", me); return -1; }
    if (!by_value && !params) { ishara_set_error("%s: null params", me); return -1; }
    if (!by_value) weights = params;
    if (!out_idx || !out_len || !out_score) { ishara_set_error("%s: null out_idx / out_len / out_score (posterior and perm may be NULL)", me); return -1; }
    uintptr_t bits = (uintptr_t)hyp_idx | (uintptr_t)hyp_len | (uintptr_t)weights | (uintptr_t)inv_temp | (uintptr_t)out_idx | (uintptr_t)out_len |
                     (uintptr_t)out_score | (uintptr_t)posterior | (uintptr_t)perm;
    for (int m = 0; m < M; ++m) bits |= (uintptr_t)logp[m];
    if (bits % 4) { ishara_set_error("%s: misaligned buffer: every buffer must be 4-byte aligned", me); return -1; }
    const size_t bn = (size_t)B * N * 4, bnt = bn * Th;
    const void* outs[5] = {out_idx, out_len, out_score, posterior, perm};
    const size_t osz[5] = {bnt, bn, bn, bn, bn};
    const char* onm[5] = {"out_idx", "out_len", "out_score", "posterior", "perm"};
    for (int o = 0; o < 5; ++o) {
        if (bytes_overlap(outs[o], osz[o], hyp_idx, bnt)) { ishara_set_error("%s: %s overlaps hyp_idx", me, onm[o]); return -1; }
        if (bytes_overlap(outs[o], osz[o], hyp_len, bn)) { ishara_set_error("%s: %s overlaps hyp_len", me, onm[o]); return -1; }
        for (int m = 0; m < M; ++m)
            if (bytes_overlap(outs[o], osz[o], logp[m], bn)) { ishara_set_error("%s: %s overlaps logp[%d]", me, onm[o], m); return -1; }
    }
    NrPtrs in;
    for (int m = 0; m < NR_MAX_M; ++m) in.p[m] = m < M ? logp[m] : nullptr;
    hipLaunchKernelGGL(nbest_rescore_kernel, dim3((unsigned)B), dim3(NR_WAVES * 64), 0, (hipStream_t)st, hyp_idx, hyp_len, N, Th, in, M, weights,
                       lm_logp, lm_next, S, start_state, C, blank, alpha, beta, by_value ? (const float*)nullptr : params + M, inv_temp, out_idx, out_len, out_score,
                       posterior, perm);
    return launch_rc();
}

extern "C" int ishara_nbest_rescore(const int32_t* hyp_idx, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Th, const float* const* logp,
                                    int32_t M, const float* weights, const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state,
                                    int32_t C, int32_t blank, float alpha, float beta, const float* inv_temp, int32_t* out_idx, int32_t* out_len,
                                    float* out_score, float* posterior, int32_t* perm, ishara_stream st) {
    return nr_run("ishara_nbest_rescore", hyp_idx, hyp_len, B, N, Th, logp, M, weights, nullptr, lm_logp, lm_next, S, start_state, C, blank, alpha, beta,
                  inv_temp, out_idx, out_len, out_score, posterior, perm, st, true);
}

extern "C" int ishara_nbest_rescore_p(const int32_t* hyp_idx, const int32_t* hyp_len, int32_t B, int32_t N, int32_t Th, const float* const* logp,
                                      int32_t M, const float* params, const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state,
                                      int32_t C, int32_t blank, const float* inv_temp, int32_t* out_idx, int32_t* out_len, float* out_score,
                                      float* posterior, int32_t* perm, ishara_stream st) {
    return nr_run("ishara_nbest_rescore_p", hyp_idx, hyp_len, B, N, Th, logp, M, nullptr, params, lm_logp, lm_next, S, start_state, C, blank, 0.f, 0.f,
                  inv_temp, out_idx, out_len, out_score, posterior, perm, st, false);
}
