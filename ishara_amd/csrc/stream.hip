// Streaming recognition beside the whole-clip wrappers: S sessions whose raw frames live on the device, one tick =
//   ishara_stream_append -> ishara_preprocess_sessions -> ishara_forward -> decode -> ishara_stream_agree
// (semantics: include/ishara_hip.h, "streaming sessions").  The three kernels here are one workgroup per session (the preprocessing: k
// per session), read every length from device memory, allocate nothing and use no atomics: each output is an exact function of the inputs.
#include "preprocess_common.h"

#define ST_THREADS 256
#define ST_WAVES (ST_THREADS / WAVE)
#define ST_CNT ISHARA_STREAM_COUNTERS
#define ST_NONE 0x7fffffff

// ---------------------------------------------------------------------------------------------------- append (steps 1 and 2 of a tick)
// The frame-by-frame rule in parallel: frames of the chunk in front of its first hand frame are dropped while the session has not started
// (h0), of the rest `fit` go into the buffer's free rows, the last hand frame among those decides `idle`.  The hand test runs once per
// stored frame (and once more per frame in front of h0): its result is the row's hand byte, which the preprocessing reads.
__global__ __launch_bounds__(ST_THREADS) void stream_append_kernel(ishara_stream_state st, const float* __restrict__ frames, int64_t n_total,
                                                                  const int64_t* __restrict__ offsets, const int* __restrict__ flags,
                                                                  int* __restrict__ fresh) {
    __shared__ int s_a[ST_WAVES], s_b[ST_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, s = blockIdx.x;
    int* cnt = st.counters + (size_t)s * ST_CNT;
    int n = cnt[0], active = cnt[1], idle = cnt[2], dropped = cnt[3], n_hist = cnt[5], clen = cnt[6];
    if ((flags[s] & ISHARA_STREAM_RESET) || cnt[4]) n = active = idle = dropped = n_hist = clen = 0;     // a finished phrase restarts by itself
    n = n < 0 ? 0 : (n > st.window ? st.window : n);       // a bad counter cannot make the kernel write outside the session's rows
    // chunk rows, clamped to the packed buffer: a bad table cannot make the kernel read outside frames
    int64_t lo = offsets[s], hi = offsets[s + 1];
    lo = lo < 0 ? 0 : (lo > n_total ? n_total : lo);
    hi = hi < lo ? lo : (hi > n_total ? n_total : hi);
    const int64_t k = hi - lo;
    const float* chunk = frames + (size_t)lo * PP_COLS;
    __syncthreads();                                       // every thread holds the counters before thread 0 rewrites them
    // ---- first hand frame of the chunk (only a session that has not started drops its leading silence)
    int64_t h0 = 0;
    if (active == 0) {
        h0 = k;
        for (int64_t f0 = 0; f0 < k; f0 += ST_THREADS) {
            const int64_t f = f0 + tid;
            const int hp = f < k && pp_hand_present(chunk + (size_t)f * PP_COLS) ? 1 : 0;
            const unsigned long long bal = __ballot(hp);
            if (lane == 0) s_a[wid] = bal ? wid * WAVE + __builtin_ctzll(bal) : ST_NONE;
            __syncthreads();
            int first = ST_NONE;
            for (int w = 0; w < ST_WAVES; ++w) first = s_a[w] < first ? s_a[w] : first;
            __syncthreads();
            if (first != ST_NONE) { h0 = f0 + first; break; }
        }
    }
    // ---- the frames that fit: hand bytes, their count, the last of them
    const int64_t avail = k - h0;
    const int room = st.window - n;
    const int fit = avail < (int64_t)room ? (int)avail : room;
    const float* src = chunk + (size_t)h0 * PP_COLS;
    uint8_t* hb = st.hand + (size_t)s * st.window + n;
    int hands = 0, last = -1;                              // wave-uniform: both come from ballots
    for (int j0 = 0; j0 < fit; j0 += ST_THREADS) {
        const int j = j0 + tid;
        const int hp = j < fit && pp_hand_present(src + (size_t)j * PP_COLS) ? 1 : 0;
        if (j < fit) hb[j] = (uint8_t)hp;
        const unsigned long long bal = __ballot(hp);
        hands += __popcll(bal);
        if (bal) last = j0 + wid * WAVE + 63 - __builtin_clzll(bal);
    }
    if (lane == 0) { s_a[wid] = hands; s_b[wid] = last; }
    __syncthreads();
    hands = 0; last = -1;
    for (int w = 0; w < ST_WAVES; ++w) { hands += s_a[w]; last = s_b[w] > last ? s_b[w] : last; }
    // ---- rows: fit * 69 float4 (a row is 1104 bytes: source and destination rows are 16-byte aligned)
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(st.raw + ((size_t)s * st.window + n) * PP_COLS);
    const size_t nq = (size_t)fit * (PP_COLS / 4);
    for (size_t q = tid; q < nq; q += ST_THREADS) d4[q] = s4[q];
    if (tid == 0) {
        cnt[0] = n + fit;
        cnt[1] = active + hands;
        cnt[2] = last >= 0 ? fit - 1 - last : idle + fit;
        cnt[3] = dropped + (int)(k - fit);
        cnt[4] = 0;
        cnt[5] = n_hist;
        cnt[6] = clen;
        fresh[s] = fit > 0 ? 1 : 0;
    }
}

// ---------------------------------------------------------------------------------------------------- preprocessing of the session buffers
// preprocess_batch_kernel (preprocess.hip) for fixed-stride buffers: session s = raw + s * window * 276, its length read from n[s * n_stride].
// With hand bytes the kept-frame list (even frame, or hand present) costs one byte per frame; without them the odd frames are tested as
// there.  Grid (k, S); all LDS is dynamic, so that its base stays 16-byte aligned: list [window rounded up to 4] | wave counts [4] | base.
__global__ __launch_bounds__(ST_THREADS) void preprocess_sessions_kernel(const float* __restrict__ raw, const int* __restrict__ n_p, int n_stride,
                                                                        const uint8_t* __restrict__ hand, int window, const float* __restrict__ mean,
                                                                        const float* __restrict__ stdv, float* __restrict__ out, int Tn) {
    extern __shared__ __attribute__((aligned(16))) int st_smem[];
    int* sh = st_smem;                                     // compacted source index list [window]
    int* s_wcnt = st_smem + ((window + 3) & ~3);
    int* s_base = s_wcnt + ST_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, b = blockIdx.y;
    int n = n_p[(size_t)b * n_stride];
    n = n < 0 ? 0 : (n > window ? window : n);
    const float* clip = raw + (size_t)b * window * PP_COLS;
    const uint8_t* hb = hand ? hand + (size_t)b * window : nullptr;
    if (tid == 0) *s_base = 0;
    __syncthreads();
    for (int f0 = 0; f0 < n; f0 += ST_THREADS) {
        const int f = f0 + tid;
        const int keep = f < n && ((f & 1) == 0 || (hb ? hb[f] != 0 : pp_hand_present(clip + (size_t)f * PP_COLS))) ? 1 : 0;
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wcnt[wid] = __popcll(bal);
        __syncthreads();
        int off = *s_base;
        for (int w = 0; w < wid; ++w) off += s_wcnt[w];
        if (keep) sh[off + before] = f;
        __syncthreads();
        if (tid == 0) { int t = 0; for (int w = 0; w < ST_WAVES; ++w) t += s_wcnt[w]; *s_base += t; }
        __syncthreads();
    }
    const int m = *s_base;
    const float ratio = m > 0 ? (float)m / (float)Tn : 1.f;
    float* o = out + (size_t)b * Tn * PP_COLS;
    const int nq = Tn * (PP_COLS / 4);
    for (int q = blockIdx.x * ST_THREADS + tid; q < nq; q += gridDim.x * ST_THREADS) {
        const int t = q / (PP_COLS / 4), c = (q - t * (PP_COLS / 4)) * 4;
        float4 v;
        v.x = pp_value(clip, sh, n, m, Tn, ratio, t, c + 0, mean, stdv);
        v.y = pp_value(clip, sh, n, m, Tn, ratio, t, c + 1, mean, stdv);
        v.z = pp_value(clip, sh, n, m, Tn, ratio, t, c + 2, mean, stdv);
        v.w = pp_value(clip, sh, n, m, Tn, ratio, t, c + 3, mean, stdv);
        *reinterpret_cast<float4*>(o + (size_t)t * PP_COLS + c) = v;
    }
}

// ---------------------------------------------------------------------------------------------------- agree (step 4 of a tick)
// Thread tid owns the columns t = tid, tid + 256, ... of the session's history, committed text and output text in every loop below, so no
// column is read by a thread other than the one that wrote it; the history's lengths (thread 0) are read behind a barrier.
__global__ __launch_bounds__(ST_THREADS) void stream_agree_kernel(ishara_stream_state st, const int* __restrict__ idx, const int* __restrict__ len,
                                                                 const int* __restrict__ flags, const int* __restrict__ fresh, int idle_frames,
                                                                 int min_active, int* __restrict__ record, int* __restrict__ text) {
    __shared__ int s_w[ST_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, s = blockIdx.x;
    const int Tn = st.T, A = st.agree;
    int* cnt = st.counters + (size_t)s * ST_CNT;
    const int n = cnt[0], active = cnt[1], idle = cnt[2], dropped = cnt[3];
    int n_hist = cnt[5], clen = cnt[6];
    n_hist = n_hist < 0 ? 0 : (n_hist > A ? A : n_hist);
    clen = clen < 0 ? 0 : (clen > Tn ? Tn : clen);
    int L = len[s];
    L = L < 0 ? 0 : (L > Tn ? Tn : L);
    const int* hyp = idx + (size_t)s * Tn;
    const int fr = fresh[s] != 0;
    const int endpoint = active >= min_active && idle >= idle_frames;
    const int full = n >= st.window;
    const int fin = (flags[s] & ISHARA_STREAM_FINISH) || full || endpoint;
    int* H = st.hist + (size_t)s * A * Tn;
    int* HL = st.hist_len + (size_t)s * A;
    int* com = st.committed + (size_t)s * Tn;
    const int clen0 = clen;
    __syncthreads();                                       // every thread holds the counters before thread 0 rewrites them
    if (fr) {
        // push: the history keeps the last A hypotheses, oldest first, each padded with -1 to T
        if (n_hist < A) {
            for (int t = tid; t < Tn; t += ST_THREADS) H[(size_t)n_hist * Tn + t] = t < L ? hyp[t] : -1;
            if (tid == 0) HL[n_hist] = L;
            ++n_hist;
        } else {
            for (int t = tid; t < Tn; t += ST_THREADS) {
                for (int i = 0; i + 1 < A; ++i) H[(size_t)i * Tn + t] = H[(size_t)(i + 1) * Tn + t];
                H[(size_t)(A - 1) * Tn + t] = t < L ? hyp[t] : -1;
            }
            if (tid == 0) { for (int i = 0; i + 1 < A; ++i) HL[i] = HL[i + 1]; HL[A - 1] = L; }
        }
        __syncthreads();
        if (n_hist == A) {
            // longest common prefix of the A hypotheses: the first column at which one of them ends or differs
            int minl = Tn;
            for (int i = 0; i < A; ++i) { const int l = HL[i]; minl = l < minl ? l : minl; }
            minl = minl < 0 ? 0 : minl;
            int l = minl;
            for (int t = tid; t < minl; t += ST_THREADS) {
                const int v = H[t];
                int same = 1;
                for (int i = 1; i < A; ++i) same &= H[(size_t)i * Tn + t] == v;
                if (!same) { l = t; break; }
            }
            for (int o = 32; o > 0; o >>= 1) { const int v = __shfl_xor(l, o); l = v < l ? v : l; }
            if (lane == 0) s_w[wid] = l;
            __syncthreads();
            l = s_w[0];
            for (int w = 1; w < ST_WAVES; ++w) l = s_w[w] < l ? s_w[w] : l;
            if (l > clen) {                                // committed symbols are never rewritten: only [clen, l) is written
                for (int t = clen + tid; t < l; t += ST_THREADS) com[t] = hyp[t];
                clen = l;
            }
        }
    }
    int* tx = text + (size_t)s * Tn;
    for (int t = tid; t < Tn; t += ST_THREADS) {
        int v = t < L ? hyp[t] : -1;
        if (!fin && t < clen) v = t >= clen0 ? hyp[t] : com[t];
        tx[t] = v;
    }
    if (tid == 0) {
        cnt[4] = fin ? 1 : 0;
        cnt[5] = n_hist;
        cnt[6] = clen;
        int* r = record + (size_t)s * ISHARA_STREAM_RECORD;
        r[0] = (fr ? ISHARA_STREAM_FRESH : 0) | (fin ? ISHARA_STREAM_FINAL : 0) | (full ? ISHARA_STREAM_FULL : 0) |
               (endpoint ? ISHARA_STREAM_ENDPOINT : 0) | (active > 0 ? ISHARA_STREAM_STARTED : 0);
        r[1] = n; r[2] = active; r[3] = idle; r[4] = dropped;
        r[5] = fin ? L : clen;
        r[6] = fin ? L : (clen > L ? clen : L);
        r[7] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------- entry points
// 0: go on; 1: nothing to do (S == 0); -1: refused (message set)
static int stream_state_check(const char* who, const ishara_stream_state* st) {
    if (!st) { ishara_set_error("%s: null state", who); return -1; }
    if (st->S < 0 || st->S > 65535) { ishara_set_error("%s: S=%d unsupported (0..65535)", who, st->S); return -1; }
    if (st->window < 1 || st->window > 8192) { ishara_set_error("%s: window %d unsupported (1..8192)", who, st->window); return -1; }
    if (st->T < 1 || st->T > 4096) { ishara_set_error("%s: T=%d unsupported (1..4096)", who, st->T); return -1; }
    if (st->agree < 2 || st->agree > 4) { ishara_set_error("%s: agree=%d unsupported (2..4)", who, st->agree); return -1; }
    if (st->S == 0) return 1;
    if (!st->raw || !st->hand || !st->counters || !st->hist || !st->hist_len || !st->committed) {
        ishara_set_error("%s: null raw / hand / counters / hist / hist_len / committed in the state", who); return -1;
    }
    if ((uintptr_t)st->raw % 16) { ishara_set_error("%s: the state's raw must be 16-byte aligned", who); return -1; }
    if (((uintptr_t)st->counters | (uintptr_t)st->hist | (uintptr_t)st->hist_len | (uintptr_t)st->committed) % 4) {
        ishara_set_error("%s: the state's int32 arrays must be 4-byte aligned", who); return -1;
    }
    return 0;
}

extern "C" int ishara_stream_append(const ishara_stream_state* st, const float* frames, int64_t n_total, const int64_t* offsets,
                                    const int32_t* flags, int32_t* fresh, ishara_stream s) {
    const int c = stream_state_check("ishara_stream_append", st);
    if (c < 0) return -1;
    if (n_total < 0) { ishara_set_error("ishara_stream_append: n_total %lld < 0", (long long)n_total); return -1; }
    if (c > 0) return 0;
    if (!offsets || !flags || !fresh || (n_total > 0 && !frames)) { ishara_set_error("ishara_stream_append: null frames / offsets / flags / fresh"); return -1; }
    if ((uintptr_t)frames % 16) { ishara_set_error("ishara_stream_append: frames must be 16-byte aligned"); return -1; }
    if ((uintptr_t)offsets % 8 || ((uintptr_t)flags | (uintptr_t)fresh) % 4) { ishara_set_error("ishara_stream_append: offsets must be 8-byte, flags and fresh 4-byte aligned"); return -1; }
    hipLaunchKernelGGL(stream_append_kernel, dim3(st->S), dim3(ST_THREADS), 0, (hipStream_t)s, *st, frames, n_total, offsets, flags, fresh);
    return launch_rc();
}

extern "C" int ishara_preprocess_sessions(const float* raw, const int32_t* n, int32_t n_stride, const uint8_t* hand, int32_t S, int32_t window,
                                          const float* mean, const float* stdv, float* out, int32_t T, ishara_stream s) {
    if (window < 1 || window > 8192) { ishara_set_error("ishara_preprocess_sessions: window %d unsupported (1..8192)", window); return -1; }
    if (S < 0 || S > 65535 || T < 1 || T > 4096) { ishara_set_error("ishara_preprocess_sessions: S=%d T=%d unsupported (0 <= S <= 65535, 1 <= T <= 4096)", S, T); return -1; }
    if (n_stride < 1) { ishara_set_error("ishara_preprocess_sessions: n_stride %d < 1", n_stride); return -1; }
    if (S == 0) return 0;
    if (!raw || !n || !mean || !stdv || !out) { ishara_set_error("ishara_preprocess_sessions: null raw / n / mean / stdv / out"); return -1; }
    if (((uintptr_t)raw | (uintptr_t)out) % 16) { ishara_set_error("ishara_preprocess_sessions: raw and out must be 16-byte aligned"); return -1; }
    if ((uintptr_t)n % 4) { ishara_set_error("ishara_preprocess_sessions: n must be 4-byte aligned"); return -1; }
    // as launch_preprocess_batch: about 1024 workgroups in all, at most 16 per session
    int k = 1024 / S;
    k = k < 1 ? 1 : (k > 16 ? 16 : k);
    const size_t lds = ((size_t)((window + 3) & ~3) + 2 * ST_WAVES) * sizeof(int);
    hipLaunchKernelGGL(preprocess_sessions_kernel, dim3(k, S), dim3(ST_THREADS), lds, (hipStream_t)s, raw, n, n_stride, hand, window, mean, stdv, out, T);
    return launch_rc();
}

extern "C" int ishara_stream_agree(const ishara_stream_state* st, const int32_t* idx, const int32_t* len, const int32_t* flags, const int32_t* fresh,
                                   int32_t idle_frames, int32_t min_active_frames, int32_t* record, int32_t* text, ishara_stream s) {
    const int c = stream_state_check("ishara_stream_agree", st);
    if (c < 0) return -1;
    if (idle_frames < 1) { ishara_set_error("ishara_stream_agree: idle_frames %d < 1", idle_frames); return -1; }
    if (min_active_frames < 0) { ishara_set_error("ishara_stream_agree: min_active_frames %d < 0", min_active_frames); return -1; }
    if (c > 0) return 0;
    if (!idx || !len || !flags || !fresh || !record || !text) { ishara_set_error("ishara_stream_agree: null idx / len / flags / fresh / record / text"); return -1; }
    if (((uintptr_t)idx | (uintptr_t)len | (uintptr_t)flags | (uintptr_t)fresh | (uintptr_t)record | (uintptr_t)text) % 4) {
        ishara_set_error("ishara_stream_agree: idx / len / flags / fresh / record / text must be 4-byte aligned"); return -1;
    }
    hipLaunchKernelGGL(stream_agree_kernel, dim3(st->S), dim3(ST_THREADS), 0, (hipStream_t)s, *st, idx, len, flags, fresh, idle_frames, min_active_frames, record, text);
    return launch_rc();
}
