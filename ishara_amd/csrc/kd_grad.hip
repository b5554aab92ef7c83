// Frame-level knowledge distillation: the gradient of a temperature-softened KL(teacher || student) with respect to the student's logits
// (ishara_kd_grad; contract in include/ishara_hip.h, host definition and float32 twin in ishara_amd/kd.py and tests/kd_parity.py).  It is
// what distillation adds to the CTC gradient: a second stage of keras_loss_backward (keras_hybrid.hip) behind the n-best stage, of the shape
// of ng_grad_kernel (ctc_nbest_grad.hip): it adds into the model's dlogits and rewrites the padded bf16 copy from the sum.
//
// One wavefront owns a frame (b, t), one lane a class; lanes >= C hold -inf for a max and 0 for a sum.  A workgroup of KD_WAVES waves takes
// KD_WAVES * KD_U consecutive frames of one clip, wave w the frames tc + w + KD_WAVES * u; the KD_U rows of both inputs (and of dlogits with
// accumulate) are loaded first, so that they are in flight together.  Every class reduction is the xor butterfly of common.h (offsets 32,
// 16, 8, 4, 2, 1: a fixed tree, every lane ends with the same bits).  Both rows go through ONE device function, so a teacher that equals the
// student bit for bit gives ps == pt and lps == lpt bit for bit: G = 0 and KL = 0 exactly.  No atomics, no workspace, no memset:
// bit-identical from run to run.  Bound by HBM: two row reads (three with accumulate), one row write and the 256-byte dlb row.
//
// Per frame t < Tb, in fp32, one rounding per operation (no FMA contraction):
//   a = z * inv_temp          ma = max a      ea = expf(a - ma)    sa = sum ea      lps = (a - ma) - logf(sa)    ps = ea / sa
//   the teacher row u the same: lpt, pt
//   KL_t = sum_c pt * (lpt - lps)             G = grad_scale * (w_b * (ps - pt)),  w_b absent in mode 0, 1 / (float)Tb in mode 1
// kl_frame leaves through LDS so that a workgroup stores its 16 values as one run; kl_clip is a second, tiny kernel (one wave per clip) that
// adds the clip's kl_frame values in ascending t from +0: a sum in that order cannot be spread over the frames' workgroups without atomics.
#include "model_types.h"
#include "ctc_lattice.h"                                // store_dlb_row

static constexpr int KD_WAVES = 4;                      // waves of a workgroup
static constexpr int KD_U = 4;                          // frames of a wave in flight together
static constexpr int KD_FRAMES = KD_WAVES * KD_U;       // frames of a workgroup

struct KdRow { float lp, p; };
// log-softmax and softmax of one tempered row held one class per lane; `on` = the lane has a class
DEVI KdRow kd_row(float z, float inv_temp, bool on) {
#pragma clang fp contract(off)
    const float a = z * inv_temp;
    const float mx = wave_max(on ? a : -INFINITY);
    const float d = a - mx;
    const float e = on ? expf(d) : 0.f;
    const float sum = wave_sum(e);
    KdRow r;
    r.lp = d - logf(sum);
    r.p = e / sum;
    return r;
}
DEVI float kd_kl_term(float pt, float lpt, float lps) {
#pragma clang fp contract(off)
    const float d = lpt - lps;
    return pt * d;
}
DEVI float kd_scaled(float grad_scale, float wb, bool mean, float ps, float pt) {
#pragma clang fp contract(off)
    const float d = ps - pt;
    const float w = mean ? wb * d : d;
    return grad_scale * w;
}
DEVI float kd_added(float old, float g) {
#pragma clang fp contract(off)
    return old + g;
}
DEVI float kd_times(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// logits and teacher may be the same buffer: neither is __restrict__
__global__ __launch_bounds__(KD_WAVES * 64) void kd_grad_kernel(const float* logits, const float* teacher, int Ts, int C, float inv_temp, int mode,
                                                                const int* __restrict__ frame_len, float grad_scale, float* __restrict__ dlogits,
                                                                int accumulate, uint32_t* __restrict__ dlb, float* __restrict__ kl_frame) {
    __shared__ float s_kl[KD_FRAMES];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int tc = blockIdx.x * KD_FRAMES;              // first frame of this workgroup
    const bool on = lane < C;
    int Tn = Ts;
    if (frame_len) Tn = frame_len[b];
    if (Tn < 1 || Tn > Ts) Tn = 0;                      // no frames: never an index or a bound
    const bool mean = mode == 1;
    const float wb = Tn > 0 ? 1.f / (float)Tn : 0.f;
    const size_t row0 = (size_t)b * Ts;
    float z[KD_U], u[KD_U], old[KD_U];
#pragma unroll
    for (int k = 0; k < KD_U; ++k) {                    // rows at or past the clip's end are read from neither input
        const int t = tc + wv + KD_WAVES * k;
        const size_t at = (row0 + t) * C + lane;
        const bool live = on && t < Tn;
        z[k] = live ? logits[at] : 0.f;
        u[k] = live ? teacher[at] : 0.f;
        old[k] = (accumulate && on && t < Ts) ? dlogits[at] : 0.f;
    }
#pragma unroll
    for (int k = 0; k < KD_U; ++k) {
        const int t = tc + wv + KD_WAVES * k;
        if (t >= Ts) continue;                          // wave-uniform
        const size_t at = (row0 + t) * C + lane;
        float gv = 0.f, kl = 0.f;
        if (t < Tn) {                                   // wave-uniform
            const KdRow s = kd_row(z[k], inv_temp, on), q = kd_row(u[k], inv_temp, on);
            kl = wave_sum(on ? kd_kl_term(q.p, q.lp, s.lp) : 0.f);
            if (on) {
                gv = kd_scaled(grad_scale, wb, mean, s.p, q.p);
                if (accumulate) gv = kd_added(old[k], gv);
                dlogits[at] = gv;
            }
        } else if (accumulate) gv = old[k];             // rows past the clip's end stay as they are
        else if (on) dlogits[at] = 0.f;
        if (lane == 0) s_kl[wv + KD_WAVES * k] = kl;
        if (dlb) store_dlb_row(dlb + (row0 + t) * 64, gv, lane);      // of the final row
    }
    if (kl_frame) {                                     // kernel-uniform
        __syncthreads();
        if (tid < KD_FRAMES && tc + tid < Ts) kl_frame[row0 + tc + tid] = s_kl[tid];
    }
}

// kl_clip[b] = kl_frame[b, 0] + kl_frame[b, 1] + ... from +0, t ascending, then * 1 / (float)Tb in mode 1; one wave per clip: 64 values are
// loaded at once and added in lane order
__global__ __launch_bounds__(64) void kd_clip_kernel(const float* __restrict__ kl_frame, int Ts, int mode, const int* __restrict__ frame_len,
                                                     float* __restrict__ kl_clip) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int Tn = Ts;
    if (frame_len) Tn = frame_len[b];
    if (Tn < 1 || Tn > Ts) Tn = 0;
    const float* row = kl_frame + (size_t)b * Ts;
    float acc = 0.f;
    for (int t0 = 0; t0 < Tn; t0 += 64) {
        const float v = t0 + lane < Tn ? row[t0 + lane] : 0.f;
        const int n = min(64, Tn - t0);
        for (int j = 0; j < n; ++j) acc = kd_added(acc, __shfl(v, j, 64));
    }
    if (mode == 1 && Tn > 0) acc = kd_times(acc, 1.f / (float)Tn);
    if (lane == 0) kl_clip[b] = acc;
}

// arguments checked by the callers (ishara_kd_grad below, ishara_loss_backward_kd in keras_hybrid.hip)
int launch_kd_grad(const float* logits, const float* teacher, int B, int T, int C, float inv_temp, int mode, const int* frame_len, float grad_scale,
                   float* dlogits, int accumulate, void* dlb, float* kl_frame, float* kl_clip, hipStream_t s) {
    const dim3 grid((unsigned)((T + KD_FRAMES - 1) / KD_FRAMES), (unsigned)B);
    hipLaunchKernelGGL(kd_grad_kernel, grid, dim3(KD_WAVES * 64), 0, s, logits, teacher, T, C, inv_temp, mode, frame_len, grad_scale, dlogits, accumulate,
                       reinterpret_cast<uint32_t*>(dlb), kl_frame);
    if (launch_rc() != 0) return -2;
    if (kl_clip) hipLaunchKernelGGL(kd_clip_kernel, dim3((unsigned)B), dim3(64), 0, s, (const float*)kl_frame, T, mode, frame_len, kl_clip);
    return launch_rc();
}

// the refusals the two entries share (me: the caller's name); 0 when the launch may go ahead (B == 0 passes and launches nothing)
int kd_grad_check(const char* me, const float* logits, const float* teacher, int B, int T, int C, float inv_temp, int mode, const int* frame_len,
                  float grad_scale, const float* dlogits, int accumulate, const void* dlb, const float* kl_frame, const float* kl_clip) {
    if (C < 2 || C > 64) { ishara_set_error("%s: C=%d outside 2..64 (one lane per class)", me, C); return -1; }
    if (T < 1 || T > 4096) { ishara_set_error("%s: T=%d outside 1..4096", me, T); return -1; }
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (B > 65535) { ishara_set_error("%s: B=%d > 65535 (one grid row per clip)", me, B); return -1; }
    if (mode != 0 && mode != 1) { ishara_set_error("%s: unknown mode %d (0 the clip's sum over frames, 1 its mean)", me, mode); return -1; }
    if (accumulate != 0 && accumulate != 1) { ishara_set_error("%s: accumulate=%d is neither 0 nor 1", me, accumulate); return -1; }
    if (!(inv_temp > 0.f) || !std::isfinite(inv_temp)) { ishara_set_error("%s: inv_temp=%g is not a finite number > 0", me, (double)inv_temp); return -1; }
    if (!std::isfinite(grad_scale)) { ishara_set_error("%s: grad_scale=%g is not finite", me, (double)grad_scale); return -1; }
    if (kl_clip && !kl_frame) { ishara_set_error("%s: kl_clip needs kl_frame (it is the sum of those values)", me); return -1; }
    if (B == 0) return 0;
    if (!logits) { ishara_set_error("%s: null logits", me); return -1; }
    if (!teacher) { ishara_set_error("%s: null teacher", me); return -1; }
    if (!dlogits) { ishara_set_error("%s: null dlogits", me); return -1; }
    if (((uintptr_t)logits | (uintptr_t)teacher | (uintptr_t)frame_len | (uintptr_t)dlogits | (uintptr_t)dlb | (uintptr_t)kl_frame | (uintptr_t)kl_clip) % 4) {
        ishara_set_error("%s: misaligned buffer: logits, teacher, frame_len, dlogits, dlb, kl_frame and kl_clip must be 4-byte aligned", me); return -1;
    }
    const size_t rows = (size_t)B * T, nin = rows * C * 4;
    struct Buf { const char* name; const void* p; size_t n; };
    const Buf in[2] = {{"logits", logits, nin}, {"teacher", teacher, nin}};
    const Buf out[4] = {{"dlogits", dlogits, nin}, {"dlb", dlb, rows * 256}, {"kl_frame", kl_frame, rows * 4}, {"kl_clip", kl_clip, (size_t)B * 4}};
    for (const Buf& o : out) {
        for (const Buf& i : in)
            if (bytes_overlap(o.p, o.n, i.p, i.n)) { ishara_set_error("%s: %s overlaps %s", me, o.name, i.name); return -1; }
        for (const Buf& o2 : out)
            if (&o2 != &o && bytes_overlap(o.p, o.n, o2.p, o2.n)) { ishara_set_error("%s: %s overlaps %s", me, o.name, o2.name); return -1; }
    }
    return 0;
}

extern "C" int ishara_kd_grad(ishara_model* prof, const float* logits, const float* teacher, int32_t B, int32_t T, int32_t C, float inv_temp, int32_t mode,
                              const int32_t* frame_len, float grad_scale, float* dlogits, int32_t accumulate, void* dlb, float* kl_frame, float* kl_clip,
                              ishara_stream st) {
    const char* me = "ishara_kd_grad";
    const int rc = kd_grad_check(me, logits, teacher, B, T, C, inv_temp, mode, frame_len, grad_scale, dlogits, accumulate, dlb, kl_frame, kl_clip);
    if (rc != 0 || B == 0) return rc;
    hipStream_t s = (hipStream_t)st;
    if (!prof) return launch_kd_grad(logits, teacher, B, T, C, inv_temp, mode, frame_len, grad_scale, dlogits, accumulate, dlb, kl_frame, kl_clip, s);
    prof->s = s;
    const double row = (double)B * T * C * 4;
    CKP(prof, "kd_grad", row * (accumulate ? 4.0 : 3.0) + (dlb ? (double)B * T * 256 : 0.0), 0,
        launch_kd_grad(logits, teacher, B, T, C, inv_temp, mode, frame_len, grad_scale, dlogits, accumulate, dlb, kl_frame, kl_clip, s));
    return 0;
}
