// Test-set scoring on the device: the edit distance behind the normalised-Levenshtein score of conv-hybrid-model.ipynb c18:1-15,
// between each clip's greedy decode (after the TFLite wrapper's len < 3 fallback, c13:22-23) and its target phrase.
//
// One wavefront per clip; lane l owns target position j = l + 1, so L <= 64 (MAX_PHRASE_LENGTH, c1:28).  The rows walk the prediction:
//   best[j] = min(prev[j-1] + (a_i != b_j), prev[j] + 1)          (substitution / deletion)
//   cur[j]  = j + min(i, min_{1<=k<=j} (best[k] - k))             (the insertion chain, cur[0] = i)
// where the running minimum is a 6-step shuffle scan across the wave.  Lanes past the target's end compute values nobody reads (the scan
// only moves upwards).  Integer arithmetic, no atomics: deterministic by construction.
#include "edit_distance.h"

#define SC_WAVES 4

__global__ __launch_bounds__(SC_WAVES * WAVE) void edit_distance_kernel(const int* __restrict__ out_idx, const int* __restrict__ out_len, int Tn,
                                                                        const int* __restrict__ targets, int L, int B,
                                                                        int* __restrict__ dist, int* __restrict__ tlen) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
    if (b >= B) return;                                    // uniform per wave
    const int j = lane + 1;
    const int bj = lane < L ? targets[(size_t)b * L + lane] : PAD_TOKEN;
    const int nb = target_length(bj);
    int na = out_len[b];
    na = na < 0 ? 0 : (na > Tn ? Tn : na);
    const bool fb = na < 3;
    if (fb) na = FALLBACK_LEN;
    const int* a = out_idx + (size_t)b * Tn;
    int p = j;                                             // row 0: prev[j] = j
    for (int i0 = 0; i0 < na; i0 += WAVE) {
        const int r_end = na - i0 < WAVE ? na - i0 : WAVE;
        const int a_lane = lane < r_end ? (fb ? fallback_phrase[i0 + lane] : a[i0 + lane]) : -1;
        for (int r = 0; r < r_end; ++r) {
            const int i = i0 + r + 1;
            const int ai = __shfl(a_lane, r);
            int left = __shfl_up(p, 1);                    // prev[j-1]
            if (lane == 0) left = i - 1;                   // prev[0]
            int v = min(left + (ai != bj ? 1 : 0), p + 1) - j;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const int o = __shfl_up(v, d);
                if (lane >= d) v = min(v, o);
            }
            p = j + min(i, v);
        }
    }
    const int last = __shfl(p, nb > 0 ? nb - 1 : 0);
    if (lane == 0) {
        dist[b] = nb > 0 ? last : na;
        tlen[b] = nb;
    }
}

int launch_edit_distance(const int* out_idx, const int* out_len, int B, int T, const int* targets, int L, int* dist, int* tlen, hipStream_t s) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(edit_distance_kernel, dim3((B + SC_WAVES - 1) / SC_WAVES), dim3(SC_WAVES * WAVE), 0, s, out_idx, out_len, T, targets, L, B, dist, tlen);
    return launch_rc();
}
