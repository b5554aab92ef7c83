// Gradient of a weighted sum of n-best CTC scores with respect to the logits (ishara_ctc_nbest_grad; contract in include/ishara_hip.h, host
// definition in ishara_amd/mwer.py): G[b, t, k] = grad_scale * sum_n coef[b, n] * (softmax(logits[b, t])[k] - post_n[b, t, k]), post_n the CTC
// class posterior of hypothesis n.  It is what minimum-risk (MWER) training adds to the CTC gradient.
//
// The lattice arithmetic is ctc_lattice.h's, as it is for ctc.hip's ctc_kernel, so N = 1, coef = 1 gives that kernel's dlogits and dlb bit
// for bit.
//
// Two kernels, nothing shared between slots, no atomics on global memory:
//   ng_lattice_kernel  grid (N, B), two waves: one slot's status (ishara_ctc_score_nbest's rule, plus bit 3 for a length above max_len), then
//                      wave 0 its alpha chain and wave 1 its beta chain, concurrently, states in registers.  The fp64 rows alpha[t][s] and
//                      bsum[t][s] go to the workspace: only the ceil(S / 64) occupied registers of the slot are written, in rows of
//                      64 * ceil((2 max_len + 1) / 64) doubles (sized by max_len, not by the width Th of the hypothesis rows).  Wave 0 leaves
//                      logp (fp64) and the slot's participation flag in the workspace's head.
//   ng_grad_kernel     grid (ceil(T / 16), B), four waves, a frame per wave at a time, four frames in flight: for n ascending over the
//                      participating slots the state posteriors exp(alpha + bsum - logp) are scatter-added to classes in LDS (ctc_kernel's
//                      phase 3: ctc_lattice.h's ctc_post_add), acc = acc + coef * (softmax - post) in unfused fp32, then
//                      dlogits (= or +=) grad_scale * acc and the padded bf16 copy of the final row.
// Workspace: 16 B * N (head, rounded up to 16) + 16 B * N * T * 64 * ceil((2 max_len + 1) / 64) bytes; every byte that is read was written by
// the same call.  DESIGN.md §4 has the figures at the training shapes.
#include <type_traits>
#include "ctc_lattice.h"

static inline size_t ng_head_bytes(int B, int N) { return (((size_t)B * N * 12) + 15) / 16 * 16; }      // logp fp64 [B N], then part int32 [B N]
size_t ctc_nbest_grad_lds_bytes(int T, int max_len) {
    const int nsr = ctc_ns(max_len), ns = nsr <= 1 ? 1 : nsr <= 2 ? 2 : nsr <= 4 ? 4 : 8;
    return (size_t)T * sizeof(float) + (size_t)64 * ns * sizeof(int);
}

// ---------------------------------------------------------------------------------------------------------------
// one slot: status, then the two recursion waves of ctc_kernel.  SPr = 64 * nsr is the run-time row stride of the workspace; NS >= nsr the
// compile-time register count of the instantiation.
template <int NS>
__global__ __launch_bounds__(128) void ng_lattice_kernel(const float* __restrict__ logits, int Ts, int C, int blank, const int* __restrict__ hyp_idx,
                                                         const int* __restrict__ hyp_len, int N, int Th, int max_len, int SPr,
                                                         const int* __restrict__ frame_len, const float* __restrict__ coef,
                                                         double* __restrict__ ws_logp, int* __restrict__ ws_part, double* __restrict__ ws_lat,
                                                         float* __restrict__ logp_out, int* __restrict__ status_out) {
    constexpr int SP = 64 * NS;
    extern __shared__ float shf[];
    float* lse = shf;                                   // [Ts]
    int* ext = reinterpret_cast<int*>(lse + Ts);        // [SP]
    const int n = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t slot = (size_t)b * N + n;
    int Tn = Ts;
    if (frame_len) Tn = frame_len[b];
    if (Tn < 1 || Tn > Ts) Tn = 0;                      // no frames: never an index or a bound
    const float cf = coef[slot];
    const bool skip = cf == 0.f;                        // +0 and -0: the slot takes no part
    if (skip && !logp_out && !status_out) {             // nobody asks for its score either: its row is not read
        if (tid == 0) { ws_part[slot] = 0; ws_logp[slot] = CTC_NEG; }
        return;
    }
    const int len = hyp_len[slot];
    const int* hyp = hyp_idx + slot * Th;
    // ishara_ctc_score_nbest's status plus the max_len limit (both waves compute it: nothing is shared before the barrier)
    const int st = ctc_hyp_status(hyp, len, Th, C, blank, Tn, lane, max_len);
    if (st) {                                           // workgroup-uniform
        if (tid == 0) {
            ws_part[slot] = 0; ws_logp[slot] = CTC_NEG;
            if (logp_out) logp_out[slot] = -INFINITY;
            if (status_out) status_out[slot] = st;
        }
        return;
    }
    const float* lg = logits + (size_t)b * Ts * C;
    double* Gw = ws_lat + slot * 2 * (size_t)Ts * SPr;  // [Ts][SPr] alpha
    double* Hw = Gw + (size_t)Ts * SPr;                 // [Ts][SPr] bsum
    for (int t = tid; t < Tn; t += 128) lse[t] = ctc_row_lse(lg + (size_t)t * C, C);
    const int S = 2 * len + 1;
    for (int s = tid; s < SP; s += 128) ext[s] = ctc_hyp_symbol(hyp, S, blank, s);      // the symbols passed the check above
    __syncthreads();

    auto recursions = [&](auto nkc) {
        ctc_lattice_waves<NS, decltype(nkc)::value>(lg, lse, ext, S, len, Tn, C, blank, Gw, Hw, SPr, lane, wave, [&](double logp) {
            if (lane == 0) {
                const bool ok = logp > -1e29;
                ws_logp[slot] = logp;
                ws_part[slot] = (ok && !skip) ? 1 : 0;
                if (logp_out) logp_out[slot] = ok ? -(float)(-logp) : -INFINITY;      // the loss writes (float)(-logp)
                if (status_out) status_out[slot] = ok ? 0 : CTC_HYP_NOALIGN;
            }
        });
    };
    const int nkb = (S + 63) >> 6;
    if (NS >= 2 && nkb == 1) recursions(std::integral_constant<int, 1>{});
    else if (NS >= 3 && nkb == 2) recursions(std::integral_constant<int, 2>{});
    else recursions(std::integral_constant<int, 0>{});
}

// ---------------------------------------------------------------------------------------------------------------
// the frames: class posteriors of every participating slot by ctc_kernel's LDS scatter-add, the weighted sum, dlogits and dlb
// The contract's arithmetic, one rounding per operation: hipcc contracts a * b + c into an FMA by default and __fmul_rn / __fadd_rn are plain
// operators in its headers, so the pragma takes the permission away (as awp.hip's awp_step)
DEVI float ng_term(float acc, float cf, float sm, float post) {
#pragma clang fp contract(off)
    const float d = sm - post;
    const float w = cf * d;
    return acc + w;
}
DEVI float ng_scaled(float grad_scale, float acc) {
#pragma clang fp contract(off)
    return grad_scale * acc;
}
DEVI float ng_added(float old, float g) {
#pragma clang fp contract(off)
    return old + g;
}
static constexpr int NG_U = 4;                          // frames of a wave in flight together, as in ctc_kernel's phase 3
template <int NS>
__global__ __launch_bounds__(256) void ng_grad_kernel(const float* __restrict__ logits, int Ts, int C, int blank, const int* __restrict__ hyp_idx,
                                                      const int* __restrict__ hyp_len, int N, int Th, int SPr, const int* __restrict__ frame_len,
                                                      const float* __restrict__ coef, float grad_scale, const double* __restrict__ ws_logp,
                                                      const int* __restrict__ ws_part, const double* __restrict__ ws_lat,
                                                      float* __restrict__ dlogits, int accumulate, uint32_t* __restrict__ dlb) {
    __shared__ float cls[4][NG_U][64];
    __shared__ float s_lse[4 * NG_U];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tc = blockIdx.x * 4 * NG_U;               // first frame of this workgroup
    int Tn = Ts;
    if (frame_len) Tn = frame_len[b];
    if (Tn < 1 || Tn > Ts) Tn = 0;
    const float* lg = logits + (size_t)b * Ts * C;
    float* dl = dlogits + (size_t)b * Ts * C;
    if (tid < 4 * NG_U && tc + tid < Tn) s_lse[tid] = ctc_row_lse(lg + (size_t)(tc + tid) * C, C);      // one thread per frame
    __syncthreads();
    float acc[NG_U], sm[NG_U];
#pragma unroll
    for (int u = 0; u < NG_U; ++u) {
        const int t = tc + wv + 4 * u;
        acc[u] = 0.f; sm[u] = 0.f;
        if (t < Tn && lane < C) sm[u] = expf(lg[(size_t)t * C + lane] - s_lse[wv + 4 * u]);
    }
    if (tc + wv < Tn) {                                 // wave-uniform: this wave has a frame of the clip
        for (int n = 0; n < N; ++n) {
            const size_t slot = (size_t)b * N + n;
            if (!ws_part[slot]) continue;               // wave-uniform
            const float cf = coef[slot];
            const double logp = ws_logp[slot];
            const int S = 2 * hyp_len[slot] + 1;        // a participating slot: 0 <= len <= max_len, S <= SPr
            const int* hyp = hyp_idx + slot * Th;
            const double* Gw = ws_lat + slot * 2 * (size_t)Ts * SPr;
            const double* Hw = Gw + (size_t)Ts * SPr;
            int exs[NS];
#pragma unroll
            for (int k = 0; k < NS; ++k) exs[k] = ctc_hyp_symbol(hyp, S, blank, lane + 64 * k);
            double al[NG_U][NS], bs[NG_U][NS];
#pragma unroll
            for (int u = 0; u < NG_U; ++u) {
                const int t = min(tc + wv + 4 * u, Tn - 1);
                cls[wv][u][lane] = 0.f;
                const double* ga = Gw + (size_t)t * SPr;
                const double* gb = Hw + (size_t)t * SPr;
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const int s = lane + 64 * k;              // strided: coalesced 512-byte reads of the lattice rows
                    al[u][k] = s < S ? ga[s] : CTC_NEG; bs[u][k] = s < S ? gb[s] : CTC_NEG;
                }
            }
#pragma unroll
            for (int u = 0; u < NG_U; ++u) {
                const int t = tc + wv + 4 * u;
                if (t >= Tn) continue;                        // wave-uniform
                ctc_post_add(cls[wv][u], [&](int k) { return exs[k]; }, S, logp, al[u], bs[u], lane);
                // the class sums were added by OTHER lanes of this wave: without the fence the compiler may hand a lane that added nothing
                // the 0 it stored itself (it did, at one register per lane)
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const float post = cls[wv][u][lane];
                acc[u] = ng_term(acc[u], cf, sm[u], post);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < NG_U; ++u) {
        const int t = tc + wv + 4 * u;
        if (t >= Ts) continue;                          // wave-uniform
        float gv = 0.f;
        if (lane < C) {
            if (t < Tn) {
                gv = ng_scaled(grad_scale, acc[u]);
                if (accumulate) gv = ng_added(dl[(size_t)t * C + lane], gv);
                dl[(size_t)t * C + lane] = gv;
            } else if (accumulate) gv = dl[(size_t)t * C + lane];      // rows past the clip's end stay as they are
            else dl[(size_t)t * C + lane] = 0.f;
        }
        if (dlb) store_dlb_row(dlb + ((size_t)b * Ts + t) * 64, gv, lane);      // of the final row
    }
}

int64_t ctc_nbest_grad_workspace_bytes(int B, int T, int N, int max_len) {
    if (B < 0 || B > 65535 || T < 1 || T > 4096 || N < 1 || N > 64 || max_len < 1 || max_len > 255) return -1;
    return (int64_t)ng_head_bytes(B, N) + (int64_t)16 * B * N * T * 64 * ctc_ns(max_len);
}

// arguments checked by the callers (ishara_ctc_nbest_grad below, ishara_loss_backward_nbest in keras_hybrid.hip)
int launch_ctc_nbest_grad(const float* logits, int B, int T, int C, int blank, const int* hyp_idx, const int* hyp_len, int N, int Th, int max_len,
                          const int* frame_len, const float* coef, float grad_scale, float* dlogits, int accumulate, void* dlb, float* logp,
                          int* status, void* ws, hipStream_t s) {
    const int nsr = ctc_ns(max_len), SPr = 64 * nsr;
    double* ws_logp = reinterpret_cast<double*>(ws);
    int* ws_part = reinterpret_cast<int*>(ws_logp + (size_t)B * N);
    double* ws_lat = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + ng_head_bytes(B, N));
    const size_t shmem = ctc_nbest_grad_lds_bytes(T, max_len);
    const dim3 g1((unsigned)N, (unsigned)B), g2((unsigned)((T + 4 * NG_U - 1) / (4 * NG_U)), (unsigned)B);
#define NG_LAUNCH(NSV) do { \
        hipLaunchKernelGGL((ng_lattice_kernel<NSV>), g1, dim3(128), shmem, s, logits, T, C, blank, hyp_idx, hyp_len, N, Th, max_len, SPr, frame_len, coef, \
                           ws_logp, ws_part, ws_lat, logp, status); \
        if (launch_rc() != 0) return -2; \
        hipLaunchKernelGGL((ng_grad_kernel<NSV>), g2, dim3(256), 0, s, logits, T, C, blank, hyp_idx, hyp_len, N, Th, SPr, frame_len, coef, grad_scale, \
                           (const double*)ws_logp, (const int*)ws_part, (const double*)ws_lat, dlogits, accumulate, reinterpret_cast<uint32_t*>(dlb)); \
    } while (0)
    if (nsr <= 1) NG_LAUNCH(1);
    else if (nsr <= 2) NG_LAUNCH(2);
    else if (nsr <= 4) NG_LAUNCH(4);
    else NG_LAUNCH(8);
#undef NG_LAUNCH
    return launch_rc();
}

extern "C" int64_t ishara_ctc_nbest_grad_workspace_bytes(int32_t B, int32_t T, int32_t N, int32_t max_len) {
    return ctc_nbest_grad_workspace_bytes(B, T, N, max_len);
}

// the refusals the two entries share (fn: the caller's name); 0 when the launch may go ahead
int ctc_nbest_grad_check(const char* me, const float* logits, int B, int T, int C, int blank, const int* hyp_idx, const int* hyp_len, int N, int Th,
                         int max_len, const int* frame_len, const float* coef, const float* dlogits, const void* dlb, const float* logp,
                         const int* status, const void* ws) {
    if (C < 2 || C > 64) { ishara_set_error("%s: C=%d outside 2..64", me, C); return -1; }
    if (T < 1 || T > 4096) { ishara_set_error("%s: T=%d outside 1..4096", me, T); return -1; }
    if (Th < 1 || Th > 4096) { ishara_set_error("%s: Th=%d outside 1..4096 (the width of the hypothesis rows)", me, Th); return -1; }
    if (N < 1 || N > 64) { ishara_set_error("%s: N=%d outside 1..64", me, N); return -1; }
    if (max_len < 1 || max_len > 255) { ishara_set_error("%s: max_len=%d outside 1..255 (the loss kernel's label limit)", me, max_len); return -1; }
    if (blank < 0 || blank >= C) { ishara_set_error("%s: blank %d outside 0..%d", me, blank, C - 1); return -1; }
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (B > 65535) { ishara_set_error("%s: B=%d > 65535 (one grid row per clip)", me, B); return -1; }
    if (B == 0) return 0;
    if (!logits || !hyp_idx || !hyp_len || !coef || !dlogits || !ws) {
        ishara_set_error("%s: null logits / hyp_idx / hyp_len / coef / dlogits / workspace (frame_len, dlb, logp and status may be NULL)", me); return -1;
    }
    if (((uintptr_t)logits | (uintptr_t)hyp_idx | (uintptr_t)hyp_len | (uintptr_t)frame_len | (uintptr_t)coef | (uintptr_t)dlogits | (uintptr_t)dlb |
         (uintptr_t)logp | (uintptr_t)status) % 4) {
        ishara_set_error("%s: misaligned buffer: every buffer must be 4-byte aligned", me); return -1;
    }
    if ((uintptr_t)ws % 16) { ishara_set_error("%s: misaligned workspace: it must be 16-byte aligned", me); return -1; }
    if (bytes_overlap(dlogits, (size_t)B * T * C * 4, logits, (size_t)B * T * C * 4)) { ishara_set_error("%s: dlogits overlaps logits", me); return -1; }
    return 0;
}

extern "C" int ishara_ctc_nbest_grad(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, const int32_t* hyp_idx,
                                     const int32_t* hyp_len, int32_t N, int32_t Th, int32_t max_len, const int32_t* frame_len, const float* coef,
                                     float grad_scale, float* dlogits, int32_t accumulate, void* dlb, float* logp, int32_t* status, void* workspace,
                                     ishara_stream st) {
    const char* me = "ishara_ctc_nbest_grad";
    if (accumulate != 0 && accumulate != 1) { ishara_set_error("%s: accumulate=%d is neither 0 nor 1", me, accumulate); return -1; }
    const int rc = ctc_nbest_grad_check(me, logits, B, T, C, blank, hyp_idx, hyp_len, N, Th, max_len, frame_len, coef, dlogits, dlb, logp, status, workspace);
    if (rc != 0 || B == 0) return rc;
    return launch_ctc_nbest_grad(logits, B, T, C, blank, hyp_idx, hyp_len, N, Th, max_len, frame_len, coef, grad_scale, dlogits, accumulate, dlb, logp,
                                 status, workspace, (hipStream_t)st);
}
