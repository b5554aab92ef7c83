// Model ensembling before the CTC decode: the frame posteriors of M <= 8 models' logits [B, T, C] fused into one normalised
// log-distribution per frame (ishara_logits_combine; contract in include/ishara_hip.h, host twin in ishara_amd/ensemble.py).
//
// One wavefront owns a row (b, t), one lane a class; lanes >= C hold -inf for a max and 0 for a sum.  A workgroup of LC_WAVES waves walks
// the rows in a grid-stride loop.  The M device pointers travel in the kernel's arguments (no pointer table in memory), weights and
// 1 / temperature are read from the device at every launch, so a captured graph follows a caller that rewrites them between replays.
// Every class reduction is the xor butterfly of common.h (a fixed tree, every lane ends with the same bits); no atomics, no workspace, no
// memset: bit-identical from run to run.  Bound by HBM: (models read + 1) * B * T * C * 4 bytes.
//
// Per row, in fp32, for the models with weight > 0 in ascending m (a model whose weight is not > 0 is not read: the branch is uniform
// over the launch):
//   z = logits_m * inv_temp[m]          lp_m = (z - max z) - log(sum exp(z - max z))
//   mode 0  s = sum_m w_m * lp_m        mode 1  s = a + log(sum_m exp(log w_m + lp_m - a)),  a = max_m (log w_m + lp_m)
//   out = s - logsumexp s               no weight > 0: s = 0, the uniform row -log C
// A row at or past its clip's frame count (frame_len outside [1, T]: no frames) is not read and is written +0.
#include "model_types.h"

static constexpr int LC_MAX_M = 8;
static constexpr int LC_WAVES = 4;                      // rows in flight per workgroup
static constexpr int LC_GRID_CAP = 4096;

struct LcPtrs { const float* p[LC_MAX_M]; };

// log-softmax of one row held one class per lane; `on` = the lane has a class
__device__ __forceinline__ float lc_log_softmax(float z, bool on) {
    const float mx = wave_max(on ? z : -INFINITY);
    const float d = z - mx;
    const float sum = wave_sum(on ? expf(d) : 0.f);
    return d - logf(sum);
}

template <int MODE, bool TEMP>
__global__ __launch_bounds__(LC_WAVES * 64) void logits_combine_kernel(LcPtrs in, int M, int64_t rows, int T, int C, const float* __restrict__ weights,
                                                                       const float* __restrict__ inv_temp, const int* __restrict__ frame_len,
                                                                       float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const bool on = lane < C;
    // the launch's weights: uniform, read once per thread
    float w[LC_MAX_M], it[LC_MAX_M];
    bool use[LC_MAX_M];
    bool any = false;
#pragma unroll
    for (int m = 0; m < LC_MAX_M; ++m) {
        w[m] = m < M ? weights[m] : 0.f;
        use[m] = w[m] > 0.f;                            // false for NaN as well
        it[m] = (TEMP && m < M) ? inv_temp[m] : 1.f;
        any = any || use[m];
        if (MODE == 1) w[m] = use[m] ? logf(w[m]) : 0.f;
    }
    const int64_t stride = (int64_t)gridDim.x * LC_WAVES;
    for (int64_t row = (int64_t)blockIdx.x * LC_WAVES + (threadIdx.x >> 6); row < rows; row += stride) {
        float* __restrict__ o = out + row * C;
        if (frame_len) {
            const int b = (int)(row / T), t = (int)(row - (int64_t)b * T);
            int tb = frame_len[b];
            if (tb < 1 || tb > T) tb = 0;
            if (t >= tb) { if (on) o[lane] = 0.f; continue; }
        }
        // the loads of every model in use first, so that they are in flight together
        float z[LC_MAX_M];
#pragma unroll
        for (int m = 0; m < LC_MAX_M; ++m) z[m] = (use[m] && on) ? in.p[m][row * C + lane] : 0.f;
        float s = 0.f;
        if (MODE == 0) {
#pragma unroll
            for (int m = 0; m < LC_MAX_M; ++m) {
                if (!use[m]) continue;
                const float lp = lc_log_softmax(TEMP ? z[m] * it[m] : z[m], on);
                s += w[m] * lp;
            }
        } else {
            float a = -INFINITY;
#pragma unroll
            for (int m = 0; m < LC_MAX_M; ++m) {
                if (!use[m]) continue;
                z[m] = w[m] + lc_log_softmax(TEMP ? z[m] * it[m] : z[m], on);      // log w_m + lp_m, kept in the model's register
                a = fmaxf(a, z[m]);
            }
            if (any) {
                float acc = 0.f;
#pragma unroll
                for (int m = 0; m < LC_MAX_M; ++m) if (use[m]) acc += expf(z[m] - a);
                s = a + logf(acc);
            }
        }
        const float r = lc_log_softmax(s, on);
        if (on) o[lane] = r;
    }
}

static int launch_logits_combine(const float* const* logits, int M, int B, int T, int C, const float* weights, const float* inv_temp, int mode,
                          const int* frame_len, float* out, hipStream_t s) {
    LcPtrs in;
    for (int m = 0; m < LC_MAX_M; ++m) in.p[m] = m < M ? logits[m] : nullptr;
    const int64_t rows = (int64_t)B * T;
    const int64_t want = (rows + LC_WAVES - 1) / LC_WAVES;
    const dim3 grid((unsigned)(want < LC_GRID_CAP ? want : LC_GRID_CAP)), block(LC_WAVES * 64);
#define LC_LAUNCH(MODE, TEMP) hipLaunchKernelGGL((logits_combine_kernel<MODE, TEMP>), grid, block, 0, s, in, M, rows, T, C, weights, inv_temp, frame_len, out)
    if (mode == 0) { if (inv_temp) LC_LAUNCH(0, true); else LC_LAUNCH(0, false); }
    else { if (inv_temp) LC_LAUNCH(1, true); else LC_LAUNCH(1, false); }
#undef LC_LAUNCH
    return launch_rc();
}

extern "C" int ishara_logits_combine(ishara_model* prof, const float* const* logits, int32_t M, int32_t B, int32_t T, int32_t C,
                                     const float* weights, const float* inv_temp, int32_t mode, const int32_t* frame_len, float* out,
                                     ishara_stream st) {
    const char* me = "ishara_logits_combine";
    if (M < 1 || M > LC_MAX_M) { ishara_set_error("%s: M=%d outside 1..%d (the models' pointers travel in the kernel's arguments)", me, M, LC_MAX_M); return -1; }
    if (C < 2 || C > 64) { ishara_set_error("%s: C=%d outside 2..64 (one lane per class)", me, C); return -1; }
    if (T < 1 || T > 4096) { ishara_set_error("%s: T=%d outside 1..4096", me, T); return -1; }
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (mode != 0 && mode != 1) { ishara_set_error("%s: unknown mode %d (0 log-linear, 1 linear)", me, mode); return -1; }
    if (B == 0) return 0;
    if (!logits) { ishara_set_error("%s: null logits", me); return -1; }
    for (int m = 0; m < M; ++m)
        if (!logits[m]) { ishara_set_error("%s: null logits[%d]", me, m); return -1; }
    if (!weights) { ishara_set_error("%s: null weights", me); return -1; }
    if (!out) { ishara_set_error("%s: null out", me); return -1; }
    uintptr_t bits = (uintptr_t)weights | (uintptr_t)inv_temp | (uintptr_t)frame_len | (uintptr_t)out;
    for (int m = 0; m < M; ++m) bits |= (uintptr_t)logits[m];
    if (bits % 4) { ishara_set_error("%s: misaligned buffer: logits[m], weights, inv_temp, frame_len and out must be 4-byte aligned", me); return -1; }
    const uintptr_t nbytes = (uintptr_t)B * T * C * 4, o0 = (uintptr_t)out;
    for (int m = 0; m < M; ++m) {
        const uintptr_t i0 = (uintptr_t)logits[m];
        if (o0 < i0 + nbytes && i0 < o0 + nbytes) { ishara_set_error("%s: out overlaps logits[%d] (%llu bytes each)", me, m, (unsigned long long)nbytes); return -1; }
    }
    hipStream_t s = (hipStream_t)st;
    if (!prof) return launch_logits_combine(logits, M, B, T, C, weights, inv_temp, mode, frame_len, out, s);
    prof->s = s;
    // the weights live on the device: the record counts every model as read (a weight that is not > 0 makes it an upper bound)
    CKP(prof, "logits_combine", ((double)M + 1.0) * (double)nbytes, 0, launch_logits_combine(logits, M, B, T, C, weights, inv_temp, mode, frame_len, out, s));
    return 0;
}
