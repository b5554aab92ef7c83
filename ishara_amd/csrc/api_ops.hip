// Entry points of libishara_hip.so that need no model handle: decoding, CTC, preprocessing, clip batches, scoring, the debug switches
// and the ishara_op_* operator entry points the tests drive single kernels through (with the two kernels only they use).
#include "model_types.h"

__global__ void dropout_mask_kernel(float* out, int rows, int cols, DropSpec d) {
    const size_t n = (size_t)rows * cols;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / cols), c = (uint32_t)(i % cols);
        out[i] = (d.thr == 0u || rng_keep(rng_row_key(d.key, r), c, d.thr)) ? d.scale : 0.f;
    }
}
// packed qkv [M,3d] (head-major) -> q,k [B,H,T,dh], vt [B,H,dh,T]   (operator tests only)
template <typename T>
__global__ void qkv_split_kernel(const T* qkv, T* q, T* k, T* vt, int B, int H, int Tn, int dh) {
    const int d = H * dh;
    const size_t n = (size_t)B * Tn * 3 * d;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t m = i / (3 * d);
        const int col = (int)(i - m * 3 * d);
        const int h = col / (3 * dh), w = col - h * 3 * dh, part = w / dh, e = w - part * dh;
        const int b = (int)(m / Tn), t = (int)(m - (size_t)b * Tn);
        const T v = qkv[i];
        if (part == 0) q[((size_t)(b * H + h) * Tn + t) * dh + e] = v;
        else if (part == 1) k[((size_t)(b * H + h) * Tn + t) * dh + e] = v;
        else vt[((size_t)(b * H + h) * dh + e) * Tn + t] = v;
    }
}

// ------------------------------------------------------------------ stand-alone entry points
// CTC loss and greedy decode: what a launch would fault or fail on is refused here, before any HIP call, each with a message of its own
// the *_ex entry points (per-sample frame counts) refuse what their fixed-T siblings refuse, through the same checks, plus a misaligned length array
static bool len_misaligned(const char* me, const char* what, const void* p) {
    if ((uintptr_t)p % 4) { ishara_set_error("%s: %s must be 4-byte aligned", me, what); return true; }
    return false;
}
static int greedy_decode_checked(const char* me, const float* logits, int B, int T, int C, int blank, int* out_idx, int* out_len, bool ex,
                                 const int* frame_len, hipStream_t s) {
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (T < 1) { ishara_set_error("%s: T=%d < 1", me, T); return -1; }
    if (T > 4096) { ishara_set_error("%s: T=%d too large (max 4096: one LDS word per frame)", me, T); return -1; }
    if (C < 1) { ishara_set_error("%s: C=%d < 1", me, C); return -1; }
    if (blank < 0 || blank >= C) { ishara_set_error("%s: blank %d outside 0..%d", me, blank, C - 1); return -1; }
    if (B == 0) return 0;
    if (!logits || !out_idx || !out_len) { ishara_set_error("%s: null logits / out_idx / out_len", me); return -1; }
    if (len_misaligned(me, "frame_len", frame_len)) return -1;
    return ex ? launch_greedy_decode_len(logits, B, T, C, blank, out_idx, out_len, frame_len, s)
              : launch_greedy_decode(logits, B, T, C, blank, out_idx, out_len, s);
}
extern "C" int ishara_greedy_decode(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, int32_t* out_idx, int32_t* out_len, ishara_stream s) {
    return greedy_decode_checked("ishara_greedy_decode", logits, B, T, C, blank, out_idx, out_len, false, nullptr, (hipStream_t)s);
}
extern "C" int ishara_greedy_decode_ex(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, int32_t* out_idx, int32_t* out_len,
                                       const int32_t* frame_len, ishara_stream s) {
    return greedy_decode_checked("ishara_greedy_decode_ex", logits, B, T, C, blank, out_idx, out_len, true, frame_len, (hipStream_t)s);
}
extern "C" int64_t ishara_ctc_workspace_bytes(int32_t B, int32_t T, int32_t L) { return (int64_t)(ctc_workspace_floats(B, T, L) * sizeof(float)); }
static int ctc_loss_checked(const char* me, const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank,
                            float* nll, float* dlogits, float grad_scale, void* ws, hipStream_t s, void* dlb, bool ex = false,
                            const int* frame_len = nullptr, const float* sample_scale = nullptr, uint32_t flags = 0) {
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (T < 1) { ishara_set_error("%s: T=%d < 1", me, T); return -1; }
    if (L < 1 || L > 255) { ishara_set_error("%s: L=%d outside 1..255 (2L+1 lattice states in at most 8 registers of a 64-lane wave)", me, L); return -1; }
    if (C < 2 || C > 64) { ishara_set_error("%s: C=%d outside 2..64 (one lane per class)", me, C); return -1; }
    if (blank < 0 || blank >= C) { ishara_set_error("%s: blank %d outside 0..%d", me, blank, C - 1); return -1; }
    if (ctc_lds_bytes(T, L) > ctc_lds_limit()) {
        ishara_set_error("%s: T=%d too large at L=%d: the kernel needs 4*T + 256*ceil((2L+1)/64) = %zu bytes of dynamic LDS, a launch grants %zu (T <= %zu)",
                         me, T, L, ctc_lds_bytes(T, L), ctc_lds_limit(), (ctc_lds_limit() - ctc_lds_bytes(0, L)) / 4);
        return -1;
    }
    if (flags & ~(uint32_t)ISHARA_CTC_ZERO_INFEASIBLE) { ishara_set_error("%s: unknown flag bits 0x%x (known: ISHARA_CTC_ZERO_INFEASIBLE = 1)", me, flags & ~(uint32_t)ISHARA_CTC_ZERO_INFEASIBLE); return -1; }
    if (B == 0) return 0;
    if (!logits || !labels || !nll || !ws) { ishara_set_error("%s: null logits / labels / nll / ws (dlogits may be NULL)", me); return -1; }
    if ((uintptr_t)ws % 8) { ishara_set_error("%s: ws must be 8-byte aligned (fp64 lattices)", me); return -1; }
    if ((uintptr_t)dlb % 4) { ishara_set_error("%s: dlb must be 4-byte aligned (packed bf16 pairs)", me); return -1; }
    if (len_misaligned(me, "frame_len", frame_len) || len_misaligned(me, "sample_scale", sample_scale)) return -1;
    if (ex) return launch_ctc_len(logits, labels, B, T, C, L, blank, nll, dlogits, grad_scale, (float*)ws, frame_len, sample_scale,
                                  (flags & ISHARA_CTC_ZERO_INFEASIBLE) ? 1 : 0, s);
    return launch_ctc(logits, labels, B, T, C, L, blank, nll, dlogits, grad_scale, (float*)ws, s, dlb);
}
extern "C" int ishara_ctc_loss_ex(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C, int32_t L, int32_t blank,
                                  float* nll, float* dlogits, float grad_scale, void* ws, const int32_t* frame_len, const float* sample_scale,
                                  uint32_t flags, ishara_stream s) {
    return ctc_loss_checked("ishara_ctc_loss_ex", logits, labels, B, T, C, L, blank, nll, dlogits, grad_scale, ws, (hipStream_t)s, nullptr, true,
                            frame_len, sample_scale, flags);
}
extern "C" int ishara_ctc_loss(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C, int32_t L, int32_t blank,
                               float* nll, float* dlogits, float grad_scale, void* ws, ishara_stream s) {
    return ctc_loss_checked("ishara_ctc_loss", logits, labels, B, T, C, L, blank, nll, dlogits, grad_scale, ws, (hipStream_t)s, nullptr);
}
// the same with the head's second output: dlb [B*T, 128] bf16, the gradient rows zero padded to 128 classes (written only with dlogits)
extern "C" int ishara_op_ctc_loss(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C, int32_t L, int32_t blank,
                                  float* nll, float* dlogits, float grad_scale, void* ws, void* dlb, ishara_stream s) {
    return ctc_loss_checked("ishara_op_ctc_loss", logits, labels, B, T, C, L, blank, nll, dlogits, grad_scale, ws, (hipStream_t)s, dlb);
}
extern "C" int ishara_dropout_mask(uint32_t seed, uint32_t site, int32_t rows, int32_t cols, float rate, float* out, ishara_stream s) {
    const DropSpec d = make_drop(seed, site, rate, true);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(1024), dim3(256), 0, (hipStream_t)s, out, rows, cols, d);
    return launch_rc();
}

static int g_dbg_epi = 0;
// bit 0: 1 register-staged NT kernel / 0 LDS-DMA NT kernel; bit 1: 1 register-transposing TN kernel; bit 2: 1 LDS-tiled dwconv; bit 3: 1 LDS-DMA 64x128 NT kernel; bits 4-7: NT ablation; bits 8-12: TN ablation; bit 13: 1 tile NT kernel instead of the A-stationary one; bits 14-15: wgrad workgroups auto / 256 / 512 / 768; bit 16: 1 two-kernel attention backward instead of the one-pass kernel
// A-stationary GEMM switches (gemm_as.hip as_default_flags: 1 paired half-line stores, 2 non-temporal side outputs, 16 / 32 chunked K = 256 / 512 form; gemm_cs.hip cs_flags: 64 the
// C-stationary route, 128 at any M); -1: library default
extern "C" int ishara_debug_set_as_flags(int32_t flags) { g_as_flags_override = flags; return 0; }
extern "C" int ishara_debug_set_nt_big(int32_t on) { g_nt_big = on; return 0; }
extern "C" int ishara_debug_force_regstage(int32_t on) { g_force_regstage = (on & 1) ? 1 : ((on >> 3) & 1 ? 2 : ((on >> 13) & 1 ? 3 : 0)); g_dbg_epi = (on >> 4) & 15; g_dbg_tn = (on >> 8) & 31; g_force_tn_regstage = (on >> 1) & 1; g_force_dw_lds = (on >> 2) & 1; { const int tb = (on >> 14) & 3; g_tn_blocks = tb == 1 ? 256 : (tb == 2 ? 512 : (tb == 3 ? 768 : 0)); } g_attn_bwd_two_pass = (on >> 16) & 1; return 0; }

extern "C" int ishara_preprocess(const float* raw, const int32_t* n_frames, int32_t max_frames, const float* mean, const float* stdv,
                                 float* out, int32_t T, ishara_stream s) {
    if (max_frames <= 0 || max_frames > 8192) { ishara_set_error("ishara_preprocess: max_frames %d unsupported (1..8192)", max_frames); return -1; }
    return launch_preprocess(raw, n_frames, max_frames, mean, stdv, out, T, (hipStream_t)s);
}
extern "C" int ishara_preprocess_batch(const float* raw, int64_t n_total, const int64_t* offsets, int32_t B, int32_t max_frames,
                                       const float* mean, const float* stdv, float* out, int32_t T, ishara_stream s) {
    if (max_frames <= 0 || max_frames > 8192) { ishara_set_error("ishara_preprocess_batch: max_frames %d unsupported (1..8192)", max_frames); return -1; }
    if (B < 0 || B > 65535 || T < 1 || T > 4096) { ishara_set_error("ishara_preprocess_batch: B=%d T=%d unsupported (0 <= B <= 65535, 1 <= T <= 4096)", B, T); return -1; }
    if (n_total < 0) { ishara_set_error("ishara_preprocess_batch: n_total %lld < 0", (long long)n_total); return -1; }
    if (B > 0 && (!offsets || !mean || !stdv || !out || (n_total > 0 && !raw))) { ishara_set_error("ishara_preprocess_batch: null raw / offsets / mean / stdv / out"); return -1; }
    if (((uintptr_t)raw | (uintptr_t)out) % 16) { ishara_set_error("ishara_preprocess_batch: raw and out must be 16-byte aligned"); return -1; }
    return launch_preprocess_batch(raw, n_total, offsets, B, max_frames, mean, stdv, out, T, (hipStream_t)s);
}
extern "C" int ishara_edit_distance(const int32_t* out_idx, const int32_t* out_len, int32_t B, int32_t T, const int32_t* targets, int32_t L,
                                    int32_t* dist, int32_t* tlen, ishara_stream s) {
    if (L < 1 || L > SCORE_MAX_L) { ishara_set_error("ishara_edit_distance: target length L=%d unsupported (1..%d: one wavefront lane per target symbol)", L, SCORE_MAX_L); return -1; }
    if (B < 0 || T < 1 || T > 4096) { ishara_set_error("ishara_edit_distance: B=%d T=%d unsupported (B >= 0, 1 <= T <= 4096)", B, T); return -1; }
    if (B > 0 && (!out_idx || !out_len || !targets || !dist || !tlen)) { ishara_set_error("ishara_edit_distance: null argument"); return -1; }
    return launch_edit_distance(out_idx, out_len, B, T, targets, L, dist, tlen, (hipStream_t)s);
}
extern "C" int64_t ishara_edit_alignment_workspace_bytes(int32_t B, int32_t T) {
    if (B < 0 || T < 1 || T > 4096) return -1;
    return (int64_t)edit_alignment_workspace_bytes(B, T);
}
extern "C" int ishara_edit_alignment(const int32_t* out_idx, const int32_t* out_len, int32_t B, int32_t T, const int32_t* targets, int32_t L,
                                     int32_t fallback, int32_t* ops, int32_t* aligned, int32_t* inserted, int32_t* confusion, void* workspace,
                                     ishara_stream s) {
    const char* me = "ishara_edit_alignment";
    if (L < 1 || L > SCORE_MAX_L) { ishara_set_error("%s: target length L=%d unsupported (1..%d: one wavefront lane per target symbol)", me, L, SCORE_MAX_L); return -1; }
    if (B < 0 || T < 1 || T > 4096) { ishara_set_error("%s: B=%d T=%d unsupported (B >= 0, 1 <= T <= 4096)", me, B, T); return -1; }
    if (B == 0) return 0;
    if (!out_idx || !out_len || !targets || !ops || !aligned || !inserted) { ishara_set_error("%s: null out_idx / out_len / targets / ops / aligned / inserted (confusion may be NULL)", me); return -1; }
    if (!workspace) { ishara_set_error("%s: null workspace (ishara_edit_alignment_workspace_bytes)", me); return -1; }
    if ((uintptr_t)workspace % 16) { ishara_set_error("%s: workspace must be 16-byte aligned (one 16-byte mask pair per table row)", me); return -1; }
    if (((uintptr_t)out_idx | (uintptr_t)out_len | (uintptr_t)targets | (uintptr_t)ops | (uintptr_t)aligned | (uintptr_t)inserted | (uintptr_t)confusion) % 4) {
        ishara_set_error("%s: int32 buffers must be 4-byte aligned", me); return -1;
    }
    return launch_edit_alignment(out_idx, out_len, B, T, targets, L, fallback, ops, aligned, inserted, confusion, workspace, (hipStream_t)s);
}
extern "C" int64_t ishara_ctc_beam_workspace_bytes(int32_t B, int32_t T, int32_t C, int32_t beam_width) {
    (void)C;
    if (B < 0 || T < 1 || T > 4096 || beam_width < 1 || beam_width > 32) return -1;
    return (int64_t)B * (int64_t)ctc_beam_workspace_words(T, beam_width) * 4;
}
// the limits every beam entry point shares; -1: refused, the message is set
static int ctc_beam_args_check(const char* me, const float* logits, int B, int T, int C, int blank, int beam_width, int nbest, float alpha, float beta,
                             void* workspace, int* out_idx, int* out_len, float* out_score, const int* frame_len) {
    if (C < 2 || C > 64) { ishara_set_error("%s: C=%d unsupported (2..64: one lane per class)", me, C); return -1; }
    if (blank < 0 || blank >= C) { ishara_set_error("%s: blank %d outside 0..%d", me, blank, C - 1); return -1; }
    if (beam_width < 1 || beam_width > 32) { ishara_set_error("%s: beam_width %d unsupported (1..32)", me, beam_width); return -1; }
    if (nbest < 1 || nbest > beam_width) { ishara_set_error("%s: nbest %d outside 1..beam_width=%d", me, nbest, beam_width); return -1; }
    if (B < 0 || B > 2147483647 / 2 || T < 1 || T > 4096) { ishara_set_error("%s: B=%d T=%d unsupported (B >= 0, 1 <= T <= 4096)", me, B, T); return -1; }
    if (!(alpha == alpha && beta == beta) || alpha - alpha != 0.0f || beta - beta != 0.0f) { ishara_set_error("%s: alpha and beta must be finite", me); return -1; }
    if (B > 0 && (!logits || !workspace || !out_idx || !out_len || !out_score)) { ishara_set_error("%s: null argument", me); return -1; }
    if ((uintptr_t)workspace % 4) { ishara_set_error("%s: workspace must be 4-byte aligned", me); return -1; }
    if (len_misaligned(me, "frame_len", frame_len)) return -1;
    return 0;
}
static int ctc_beam_checked(const char* me, const float* logits, int B, int T, int C, int blank, int beam_width, int nbest, const float* lm,
                            float alpha, float beta, void* workspace, int* out_idx, int* out_len, float* out_score, bool ex, const int* frame_len,
                            hipStream_t s) {
    if (ctc_beam_args_check(me, logits, B, T, C, blank, beam_width, nbest, alpha, beta, workspace, out_idx, out_len, out_score, frame_len)) return -1;
    return ex ? launch_ctc_beam_len(logits, B, T, C, blank, beam_width, nbest, lm, alpha, beta, workspace, out_idx, out_len, out_score, frame_len, s)
              : launch_ctc_beam(logits, B, T, C, blank, beam_width, nbest, lm, alpha, beta, workspace, out_idx, out_len, out_score, s);
}
extern "C" int ishara_ctc_beam_decode(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, int32_t beam_width, int32_t nbest,
                                      const float* lm, float alpha, float beta, void* workspace,
                                      int32_t* out_idx, int32_t* out_len, float* out_score, ishara_stream s) {
    return ctc_beam_checked("ishara_ctc_beam_decode", logits, B, T, C, blank, beam_width, nbest, lm, alpha, beta, workspace, out_idx, out_len,
                            out_score, false, nullptr, (hipStream_t)s);
}
extern "C" int ishara_ctc_beam_decode_ex(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, int32_t beam_width, int32_t nbest,
                                         const float* lm, float alpha, float beta, void* workspace,
                                         int32_t* out_idx, int32_t* out_len, float* out_score, const int32_t* frame_len, ishara_stream s) {
    return ctc_beam_checked("ishara_ctc_beam_decode_ex", logits, B, T, C, blank, beam_width, nbest, lm, alpha, beta, workspace, out_idx, out_len,
                            out_score, true, frame_len, (hipStream_t)s);
}
extern "C" int ishara_ctc_beam_decode_lm(const float* logits, int32_t B, int32_t T, int32_t C, int32_t blank, int32_t beam_width, int32_t nbest,
                                         const float* lm_logp, const int32_t* lm_next, int32_t S, int32_t start_state, float alpha, float beta,
                                         void* workspace, int32_t* out_idx, int32_t* out_len, float* out_score, const int32_t* frame_len,
                                         ishara_stream s) {
    const char* me = "ishara_ctc_beam_decode_lm";
    if (ctc_beam_args_check(me, logits, B, T, C, blank, beam_width, nbest, alpha, beta, workspace, out_idx, out_len, out_score, frame_len)) return -1;
    if (S < 1 || S > (1 << 22)) { ishara_set_error("%s: S=%d states unsupported (1..2^22)", me, S); return -1; }
    if (start_state < 0 || start_state >= S) { ishara_set_error("%s: start_state %d outside 0..%d", me, start_state, S - 1); return -1; }
    if (B > 0 && (!lm_logp || !lm_next)) { ishara_set_error("%s: null lm_logp / lm_next (the table entry points take a NULL lm)", me); return -1; }
    if (((uintptr_t)lm_logp | (uintptr_t)lm_next) % 16) { ishara_set_error("%s: lm_logp and lm_next must be 16-byte aligned", me); return -1; }
    return launch_ctc_beam_lm(logits, B, T, C, blank, beam_width, nbest, lm_logp, lm_next, S, start_state, alpha, beta, workspace, out_idx, out_len,
                              out_score, frame_len, (hipStream_t)s);
}
// CTC forced alignment: refused before any HIP call, as the loss is
extern "C" int64_t ishara_ctc_align_workspace_bytes(int32_t B, int32_t T, int32_t L) {
    if (B < 0 || T < 1 || T > 4096 || L < 1 || L > 255) return -1;
    return (int64_t)ctc_align_workspace_bytes(B, T, L);
}
static int ctc_align_checked(const char* me, const float* logits, const int64_t* labels, int B, int T, int C, int L, int blank, void* ws,
                             int* frame_pos, int* start, int* end, float* conf, float* score, bool ex, const int* frame_len, hipStream_t s) {
    if (B < 0) { ishara_set_error("%s: B=%d < 0", me, B); return -1; }
    if (T < 1 || T > 4096) { ishara_set_error("%s: T=%d outside 1..4096", me, T); return -1; }
    if (L < 1 || L > 255) { ishara_set_error("%s: L=%d outside 1..255 (2L+1 lattice states in at most 8 registers of a 64-lane wave)", me, L); return -1; }
    if (C < 2 || C > 64) { ishara_set_error("%s: C=%d outside 2..64", me, C); return -1; }
    if (blank < 0 || blank >= C) { ishara_set_error("%s: blank %d outside 0..%d", me, blank, C - 1); return -1; }
    if (B == 0) return 0;
    if (!logits || !labels || !ws || !frame_pos || !start || !end || !conf || !score) {
        ishara_set_error("%s: null logits / labels / ws / frame_pos / start / end / conf / score", me); return -1;
    }
    if ((uintptr_t)ws % 16) { ishara_set_error("%s: ws must be 16-byte aligned", me); return -1; }
    if (len_misaligned(me, "frame_len", frame_len)) return -1;
    return ex ? launch_ctc_align_len(logits, labels, B, T, C, L, blank, ws, frame_pos, start, end, conf, score, frame_len, s)
              : launch_ctc_align(logits, labels, B, T, C, L, blank, ws, frame_pos, start, end, conf, score, s);
}
extern "C" int ishara_ctc_align(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C, int32_t L, int32_t blank,
                                void* ws, int32_t* frame_pos, int32_t* start, int32_t* end, float* conf, float* score, ishara_stream s) {
    return ctc_align_checked("ishara_ctc_align", logits, labels, B, T, C, L, blank, ws, frame_pos, start, end, conf, score, false, nullptr, (hipStream_t)s);
}
extern "C" int ishara_ctc_align_ex(const float* logits, const int64_t* labels, int32_t B, int32_t T, int32_t C, int32_t L, int32_t blank,
                                   void* ws, int32_t* frame_pos, int32_t* start, int32_t* end, float* conf, float* score,
                                   const int32_t* frame_len, ishara_stream s) {
    return ctc_align_checked("ishara_ctc_align_ex", logits, labels, B, T, C, L, blank, ws, frame_pos, start, end, conf, score, true, frame_len, (hipStream_t)s);
}
extern "C" int ishara_clip_batch(const float* raw, const ishara_clip_aug* clips, int32_t B, int32_t T, int32_t layout,
                                 float* x, ishara_stream s) {
    if (B < 0 || T < 1 || T > CLIP_MAX_T) { ishara_set_error("ishara_clip_batch: B=%d T=%d unsupported (B >= 0, 1 <= T <= %d)", B, T, CLIP_MAX_T); return -1; }
    if (layout != ISHARA_LAYOUT_FLAT && layout != ISHARA_LAYOUT_HANDS_LIPS_XY) { ishara_set_error("ishara_clip_batch: unknown layout %d", layout); return -1; }
    if (B > 0 && (!clips || !x)) { ishara_set_error("ishara_clip_batch: null clips / x"); return -1; }
    if (((uintptr_t)raw | (uintptr_t)x) % 16) { ishara_set_error("ishara_clip_batch: raw and x must be 16-byte aligned"); return -1; }
    return launch_clip_batch(raw, clips, B, T, layout, x, (hipStream_t)s);
}
extern "C" int ishara_clip_batch_ex(const float* raw, const ishara_clip_aug_ex* clips, int32_t B, int32_t T, int32_t layout,
                                    float* x, int32_t* frame_len, ishara_stream s) {
    if (B < 0 || T < 1 || T > CLIP_MAX_T) { ishara_set_error("ishara_clip_batch_ex: B=%d T=%d unsupported (B >= 0, 1 <= T <= %d)", B, T, CLIP_MAX_T); return -1; }
    if (layout != ISHARA_LAYOUT_FLAT && layout != ISHARA_LAYOUT_HANDS_LIPS_XY) { ishara_set_error("ishara_clip_batch_ex: unknown layout %d", layout); return -1; }
    if (B > 0 && (!clips || !x)) { ishara_set_error("ishara_clip_batch_ex: null clips / x"); return -1; }
    if (((uintptr_t)raw | (uintptr_t)x) % 16) { ishara_set_error("ishara_clip_batch_ex: raw and x must be 16-byte aligned"); return -1; }
    return launch_clip_batch_ex(raw, clips, B, T, layout, x, frame_len, (hipStream_t)s);
}

// ---- operator tests: dense
// every operator entry point checks its dtype first: ISHARA_F32 / BF16 / F16 known, F16 only where an fp16 kernel exists (forward /
// inference: the backward operators refuse it); nothing is launched for a refused call
static bool op_dt_ok(const char* op, int dt, bool f16_ok) {
    if (dt != DT_F32 && dt != DT_BF16 && dt != DT_F16) { ishara_set_error("%s: unknown dtype %d (ISHARA_F32 = 0, ISHARA_BF16 = 1, ISHARA_F16 = 2)", op, dt); return false; }
    if (dt == DT_F16 && !f16_ok) { ishara_set_error("%s: ISHARA_F16 is inference-only (no fp16 backward kernels)", op); return false; }
    return true;
}
#define OP_DT(op, dt, f16_ok) do { if (!op_dt_ok(op, dt, f16_ok)) return -1; } while (0)
// the weight shadows of one Dense [K, N] at the head of an operator's scratch: Wt | Wn | wgrad slab (byte offsets wt, wn, slab; total bytes)
struct OpShadow {
    size_t wt, wn, slab, total; int ldt, ldn;
    OpShadow(int dt, int K, int N, int M) {
        const int bk = dt_is16(dt) ? 64 : 32;      // the K tile the model's shadows use (plan_shadow): 64 for both 16-bit types
        const size_t es = dt_size(dt);
        ldt = (int)rup(K, bk); ldn = (int)rup(N, bk);
        wt = 0;
        wn = rup(rup(N, 128) * (size_t)ldt * es, 256);
        slab = wn + rup(rup(K, 128) * (size_t)ldn * es, 256);
        total = slab + gemm_tn_slab_floats(M, K, N, dt) * sizeof(float);
    }
    // zero-fills both shadows (their padding) and writes W into them
    int build(int dt, const float* Wm, int K, int N, char* sc, hipStream_t s) const {
        HIP_CHECK_RET(hipMemsetAsync(sc, 0, slab, s));
        return launch_make_shadow(dt, Wm, K, N, sc + wt, ldt, sc + wn, ldn, s);
    }
};
extern "C" int64_t ishara_op_scratch_bytes(int32_t M, int32_t K, int32_t N) {
    return (int64_t)OpShadow(DT_F32, K, N, M).total;      // (the f32 layout is the largest: 4-byte elements, K tile >= half the 16-bit one)
}
extern "C" int ishara_op_dense_fwd(int32_t dt, const void* x, const float* Wm, const float* bias, void* y, int32_t M, int32_t K, int32_t N, int32_t act, void* scratch, ishara_stream st) {
    OP_DT("ishara_op_dense_fwd", dt, true);
    hipStream_t s = (hipStream_t)st;
    const OpShadow sh(dt, K, N, M);
    char* sc = (char*)scratch;
    CK(sh.build(dt, Wm, K, N, sc, s));
    OpArgs no; EpiArgs ea; ea.bias = bias; ea.act = act; ea.dbg = g_dbg_epi;
    return launch_gemm_nt(dt, dt, dt, OP_NONE, x, sc + sh.wt, y, M, N, K, sh.ldt, no, ea, s);
}
// y = act(x @ W + b) + resid
extern "C" int ishara_op_dense_fwd_ex(int32_t dt, const void* x, const float* Wm, const float* bias, const void* resid, void* y,
                                      int32_t M, int32_t K, int32_t N, int32_t act, void* scratch, ishara_stream st) {
    OP_DT("ishara_op_dense_fwd_ex", dt, true);
    hipStream_t s = (hipStream_t)st;
    const OpShadow sh(dt, K, N, M);
    char* sc = (char*)scratch;
    CK(sh.build(dt, Wm, K, N, sc, s));
    OpArgs no; EpiArgs ea; ea.bias = bias; ea.act = act; ea.resid = resid; ea.dbg = g_dbg_epi;
    return launch_gemm_nt(dt, dt, dt, OP_NONE, x, sc + sh.wt, y, M, N, K, sh.ldt, no, ea, s);
}
// the profiler key (= rocprof name prefix) of the kernel ishara_op_dense_fwd_ex runs for these arguments under the current switches: host only,
// nothing is launched — so a test can tell WHICH kernel a route decision picks when two routes give identical outputs
extern "C" const char* ishara_debug_dense_kernel_name(int32_t dt, int32_t M, int32_t K, int32_t N, int32_t act, int32_t with_resid) {
    if (!op_dt_ok("ishara_debug_dense_kernel_name", dt, true) || M < 1 || K < 1 || N < 1) return "";
    const OpShadow sh(dt, K, N, M);
    const void* aligned = reinterpret_cast<const void*>(uintptr_t(256));      // stands for 16-byte aligned operands; never dereferenced
    EpiArgs ea; ea.bias = reinterpret_cast<const float*>(aligned); ea.act = act; ea.resid = with_resid ? aligned : nullptr; ea.dbg = g_dbg_epi;
    return gemm_nt_kernel_name(dt, dt, dt, OP_NONE, aligned, M, N, K, sh.ldt, ea);
}
// the same for the depthwise conv: the kernel launch_dwconv_fwd (backward != 0: launch_dwconv_bwd_bn / launch_dwconv_bwd) runs for these
// arguments under the current switches, a two-pass backward as "dgrad+wgrad", "" for a refused call.  flags: 1 statistics wanted, 2 scratch
// given, 4 BatchNorm backward folded in (launch_dwconv_bwd_bn).  Host only: nothing is launched.  The answer is valid until the next call
extern "C" const char* ishara_debug_dwconv_kernel_name(int32_t dt, int32_t backward, int32_t B, int32_t T, int32_t C, int32_t k, int32_t padl, int32_t flags) {
    if (!op_dt_ok("ishara_debug_dwconv_kernel_name", dt, !backward) || B < 1 || T < 1 || C < 1) return "";
    if (backward) return dwconv_bwd_kernel_name(dt, C, k, padl, (flags & 2) != 0, (flags & 4) != 0);
    return dwconv_fwd_kernel_name(dt, B, T, C, k, (flags & 1) != 0, (flags & 2) != 0);
}
// the same for the attention: the kernel launch_attn_fwd (backward != 0: launch_attn_bwd) runs for these arguments under the current switches,
// with its template arguments, a kernel pair as "dq + dkv<...>", "" for a refused call.  impl: 0 / 1 as the launchers take it.  flags: 1 dropout
// active, 2 keep-bit buffer given, 4 head-major dqkv, 8 masked (a bias table or key lengths given).  Host only: nothing is launched.  The answer is valid until the next call
extern "C" const char* ishara_debug_attn_kernel_name(int32_t dt, int32_t backward, int32_t T, int32_t dh, int32_t impl, int32_t flags) {
    if (!op_dt_ok("ishara_debug_attn_kernel_name", dt, true) || T < 1) return "";
    if (backward) return attn_bwd_kernel_name(dt, T, dh, impl, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0);
    return attn_fwd_kernel_name(dt, T, dh, impl, (flags & 1) != 0, (flags & 2) != 0, (flags & 8) != 0);
}
// the same for a Conv1DBlock of the Keras hybrid: the launch plan conv_fwd / conv_bwd (conv_block.hip) run for a block of width d and kernel size k
// at (B, T) under the current switches, as "forward|backward" text (conv_block_route_name), "" for a refused dtype or shape.  flags: 1 drop-path
// active, 2 frame lengths given, 4 the per-sample-affine weight gradient switched on (the model: bf16 and no ISHARA_NO_PSA).  The project conv's
// shadow strides follow the model's rule (shadow_ld).  Host only: nothing is launched.  The answer is valid until this thread's next call
extern "C" const char* ishara_debug_conv_block_route_name(int32_t dt, int32_t training, int32_t B, int32_t T, int32_t d, int32_t k, int32_t flags) {
    if (!op_dt_ok("ishara_debug_conv_block_route_name", dt, !training) || B < 1 || T < 1 || d < 1) return "";
    if ((dt == DT_F16 && (flags & 2)) || (!training && (flags & 1))) return "";      // no frame lengths in fp16, no drop-path at inference
    return conv_block_route_name(conv_block_plan(dt, training != 0, B, T, d, k, shadow_ld(dt, 2 * d), shadow_ld(dt, d), (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0), training != 0);
}
extern "C" int ishara_op_dense_bwd(int32_t dt, const void* x, const float* Wm, const void* dy, void* dx, float* dW, float* db,
                                   int32_t M, int32_t K, int32_t N, void* scratch, ishara_stream st) {
    OP_DT("ishara_op_dense_bwd", dt, false);
    hipStream_t s = (hipStream_t)st;
    const OpShadow sh(dt, K, N, M);
    char* sc = (char*)scratch;
    CK(sh.build(dt, Wm, K, N, sc, s));
    OpArgs no; EpiArgs ea;
    if (dx) CK(launch_gemm_nt(dt, dt, dt, OP_NONE, dy, sc + sh.wn, dx, M, K, N, sh.ldn, no, ea, s));
    return launch_gemm_tn(dt, dt, dt, OP_NONE, OP_NONE, x, dy, dW, db, (float*)(sc + sh.slab), M, K, N, no, no, s);
}
// QKV projection of the attention module at inference (mhsa_fwd): LayerNorm (gamma NULL: none), x @ W + b, and the EPI_QKV scatter into
// q, k [B,H,T,dh] and vt [B,H,dh,T].  scratch: the weight shadow, then the LayerNorm output and its row statistics where the LayerNorm
// runs as a kernel of its own
static void qkv_scratch_layout(int B, int T, int H, int dh, size_t& xn, size_t& mean, size_t& rstd, size_t& total) {
    const int M = B * T, d = H * dh;
    xn = rup(OpShadow(DT_F32, d, 3 * d, M).total, 256);
    mean = xn + rup((size_t)M * d * 4, 256);
    rstd = mean + rup((size_t)M * 4, 256);
    total = rstd + rup((size_t)M * 4, 256);
}
extern "C" int64_t ishara_op_qkv_scratch_bytes(int32_t B, int32_t T, int32_t H, int32_t dh) {
    if (B < 1 || T < 1 || H < 1 || dh < 1) return -1;
    size_t xn, mean, rstd, total;
    qkv_scratch_layout(B, T, H, dh, xn, mean, rstd, total);
    return (int64_t)total;
}
extern "C" int ishara_op_qkv_fwd(int32_t dt, const void* x, const float* gamma, const float* beta, float eps, const float* Wm, const float* bias,
                                 void* q, void* k, void* vt, int32_t B, int32_t T, int32_t H, int32_t dh, int32_t head_major, void* scratch, ishara_stream st) {
    OP_DT("ishara_op_qkv_fwd", dt, true);
    if (B < 1 || T < 1 || H < 1 || dh < 1 || T % 8 != 0 || dh % 8 != 0 || (head_major != 0 && head_major != 1)) {
        ishara_set_error("ishara_op_qkv_fwd: B=%d T=%d H=%d dh=%d head_major=%d unsupported (T, dh multiples of 8; head_major 0 / 1)", B, T, H, dh, head_major); return -1;
    }
    const int d = H * dh, M = B * T;
    if ((gamma != nullptr) != (beta != nullptr) || (gamma && d > 512)) { ishara_set_error("ishara_op_qkv_fwd: LayerNorm needs both gamma and beta and H*dh <= 512 (H*dh=%d)", d); return -1; }
    if (!x || !Wm || !q || !k || !vt || !scratch || ((uintptr_t)x | (uintptr_t)scratch) % 16 != 0) { ishara_set_error("ishara_op_qkv_fwd: null or misaligned buffer (x, scratch: 16-byte aligned)"); return -1; }
    hipStream_t s = (hipStream_t)st;
    const OpShadow sh(dt, d, 3 * d, M);
    char* sc = (char*)scratch;
    CK(sh.build(dt, Wm, d, 3 * d, sc, s));
    OpArgs no;
    EpiArgs eq; eq.mode = EPI_QKV; eq.q = q; eq.k = k; eq.vt = vt; eq.H = H; eq.dh = dh; eq.T = T; eq.head_major = head_major;
    const void* A = x;
    if (gamma && !ln_as_prologue(dt, M, 3 * d, d, sh.ldt, gamma, beta, eps, nullptr, nullptr, nullptr, eq)) {      // the model's decision (ln_prologue)
        size_t xn, mean, rstd, tot;
        qkv_scratch_layout(B, T, H, dh, xn, mean, rstd, tot);
        CK(launch_layernorm_fwd(dt, x, gamma, beta, eps, sc + xn, (float*)(sc + mean), (float*)(sc + rstd), M, d, s));
        A = sc + xn;
    }
    eq.bias = bias;
    return launch_gemm_nt(dt, dt, dt, OP_NONE, A, sc + sh.wt, nullptr, M, 3 * d, d, sh.ldt, no, eq, s);
}
// the head's classifier: fp32 logits [M, C] = x [M, K] @ W [K, C] + b through `route` (classifier_fwd; 0 = the model's choice)
extern "C" int ishara_op_classifier_fwd(int32_t dt, const void* x, const float* Wm, const float* bias, float* logits, int32_t M, int32_t K, int32_t C,
                                        int32_t route, void* scratch, ishara_stream st) {
    OP_DT("ishara_op_classifier_fwd", dt, true);
    if (route < CLS_AUTO || route > CLS_GEMM) { ishara_set_error("ishara_op_classifier_fwd: unknown route %d (0 auto, 1 A-stationary, 2 dense_narrow, 3 GEMM)", route); return -1; }
    if (M < 1 || K < 1 || C < 1) { ishara_set_error("ishara_op_classifier_fwd: bad shape M=%d K=%d C=%d", M, K, C); return -1; }
    const int r = route == CLS_AUTO ? cls_route_auto(dt, M, K, C) : route;
    const char* why = nullptr;
    if (r != CLS_GEMM && !dt_is16(dt)) why = "16-bit operands only";
    else if (r == CLS_AS && (C > 64 || C % 4 != 0 || (K != 256 && K != 512))) why = "C <= 64, C % 4 == 0 and K 256 / 512 only";
    else if (r == CLS_AS && g_force_regstage) why = "the A-stationary kernel is switched off (ishara_debug_force_regstage)";
    else if (r == CLS_NARROW && (C > 64 || K % 32 != 0)) why = "C <= 64 and K % 32 == 0 only";
    else if (r == CLS_GEMM && K % (dt_is16(dt) ? 8 : 4) != 0) why = "16-byte operand rows only";
    if (why) { ishara_set_error("ishara_op_classifier_fwd: route %d does not take dt=%d M=%d K=%d C=%d: %s", r, dt, M, K, C, why); return -1; }
    if (!x || !Wm || !logits || !scratch || ((uintptr_t)x | (uintptr_t)scratch) % 16 != 0) { ishara_set_error("ishara_op_classifier_fwd: null or misaligned buffer (x, scratch: 16-byte aligned)"); return -1; }
    hipStream_t s = (hipStream_t)st;
    const OpShadow sh(dt, K, C, M);      // rup(C, 128) >= 64 zero-filled shadow rows: the N = 64 A-stationary route reads them
    char* sc = (char*)scratch;
    CK(sh.build(dt, Wm, K, C, sc, s));
    return classifier_fwd(nullptr, r, dt, x, sc + sh.wt, sh.ldt, bias, logits, M, K, C, s);
}
// row log-softmax over fp32 logits and its backward: the output layer of the torch Squeezeformer (squeezeformer/model.py:448-449)
extern "C" int ishara_op_log_softmax_fwd(const float* x, float* y, int32_t M, int32_t C, int32_t ld, ishara_stream s) { return launch_log_softmax_fwd(x, y, M, C, ld, (hipStream_t)s); }
extern "C" int ishara_op_log_softmax_bwd(const float* dy, const float* y, float* dx, int32_t M, int32_t C, int32_t ld, ishara_stream s) { return launch_log_softmax_bwd(dy, y, dx, M, C, ld, (hipStream_t)s); }
extern "C" int ishara_op_layernorm_fwd(int32_t dt, const void* x, const float* gamma, const float* beta, float eps, void* y, float* mean, float* rstd, int32_t M, int32_t C, ishara_stream s) {
    OP_DT("ishara_op_layernorm_fwd", dt, true);
    return launch_layernorm_fwd(dt, x, gamma, beta, eps, y, mean, rstd, M, C, (hipStream_t)s);
}
extern "C" int ishara_op_layernorm_bwd(int32_t dt, const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, void* dx, float* dgamma, float* dbeta, int32_t M, int32_t C, ishara_stream s) {
    OP_DT("ishara_op_layernorm_bwd", dt, false);
    return launch_layernorm_bwd(dt, dy, x, mean, rstd, gamma, nullptr, dx, dgamma, dbeta, nullptr, M, C, (hipStream_t)s);
}
extern "C" int ishara_op_dwconv_fwd(int32_t dt, int32_t inop, const void* x, const float* w, const float* bias, void* y, float* ssum, float* ssq,
                                    int32_t B, int32_t T, int32_t C, int32_t k, int32_t padl, ishara_stream s) {
    OP_DT("ishara_op_dwconv_fwd", dt, true);
    return launch_dwconv_fwd(dt, inop, x, w, bias, y, ssum, ssq, nullptr, B, T, C, k, padl, (hipStream_t)s);
}
// the same with caller scratch for the deterministic statistics (partial rows summed in a fixed order): the path the model takes, and the
// only one that reaches the streaming K = 11 / 15 kernel at B > 8
extern "C" int64_t ishara_op_dwconv_fwd_scratch_bytes(int32_t B, int32_t T, int32_t C) { return (int64_t)(dwconv_fwd_scratch_floats(B, T, C) * sizeof(float)); }
extern "C" int ishara_op_dwconv_fwd_ex(int32_t dt, int32_t inop, const void* x, const float* w, const float* bias, void* y, float* ssum, float* ssq,
                                       void* scratch, int32_t B, int32_t T, int32_t C, int32_t k, int32_t padl, ishara_stream s) {
    OP_DT("ishara_op_dwconv_fwd_ex", dt, true);
    return launch_dwconv_fwd(dt, inop, x, w, bias, y, ssum, ssq, (float*)scratch, B, T, C, k, padl, (hipStream_t)s);
}
extern "C" int64_t ishara_op_dwconv_scratch_bytes(int32_t C, int32_t k) { return (int64_t)(dwconv_bwd_scratch_floats(C, k) * sizeof(float)); }
// the depthwise-conv backward operators: everything a launch would fault or fail on is refused here, before any HIP call, each with a
// message of its own.  `required` / `optional`: operands that must not / may be NULL; all of them 16-byte aligned (vector loads and stores)
static int dwconv_bwd_refused(const char* me, int dt, int B, int T, int C, int k, int padl, std::initializer_list<const void*> required,
                              std::initializer_list<const char*> names, std::initializer_list<const void*> optional) {
    if (B < 1 || T < 1) { ishara_set_error("%s: B=%d T=%d: B and T must be >= 1", me, B, T); return -1; }
    if (B > 65535) { ishara_set_error("%s: B=%d too large (B <= 65535: one grid row per sample)", me, B); return -1; }
    if (C < 8 || C % 8 != 0) { ishara_set_error("%s: C=%d must be a positive multiple of 8", me, C); return -1; }
    if (dwconv_bwd_route(dt, C, k, 0, false, false).kind == DWB_REFUSED) { ishara_set_error("%s: kernel size %d unsupported (1..%d)", me, k, DW_MAXK); return -1; }
    if (padl < 0 || padl >= k) { ishara_set_error("%s: padl=%d outside 0..%d (the left padding of a %d-tap kernel)", me, padl, k - 1, k); return -1; }
    for (size_t i = 0; i < required.size(); ++i) if (!required.begin()[i]) { ishara_set_error("%s: null %s", me, names.begin()[i]); return -1; }
    for (size_t i = 0; i < required.size(); ++i)
        if ((uintptr_t)required.begin()[i] % 16) { ishara_set_error("%s: misaligned %s: 16-byte aligned operands (vector loads and stores)", me, names.begin()[i]); return -1; }
    uintptr_t opt = 0;
    for (const void* p : optional) opt |= (uintptr_t)p;
    if (opt % 16) { ishara_set_error("%s: misaligned optional operand (dbias / scratch / sg): 16-byte aligned operands (vector loads and stores)", me); return -1; }
    return 0;
}
extern "C" int ishara_op_dwconv_bwd(int32_t dt, int32_t inop, const void* dy, const void* x, const float* w, void* dx, float* dw, float* dbias,
                                    void* scratch, int32_t B, int32_t T, int32_t C, int32_t k, int32_t padl, ishara_stream s) {
    OP_DT("ishara_op_dwconv_bwd", dt, false);
    if (dwconv_bwd_refused("ishara_op_dwconv_bwd", dt, B, T, C, k, padl, {dy, x, w, dx, dw}, {"dy", "x", "w", "dx", "dw"}, {dbias, scratch})) return -1;
    return launch_dwconv_bwd(dt, inop, dy, x, w, dx, dw, dbias, (float*)scratch, B, T, C, k, padl, (hipStream_t)s);
}
// dx [B,T,C] (dt) = a[c] * (dy * sg[b,c] + E[b or 0, c] - (h - mean[c]) * rstd[c] * Fc[c]): the BatchNorm backward as a launch of its own
extern "C" int ishara_op_bn_bwd_apply(int32_t dt, const void* dy, const void* h, const float* mean, const float* rstd, const float* a, const float* sg,
                                      const float* E, int32_t e_per_sample, const float* Fc, void* dx, int32_t B, int32_t T, int32_t C, ishara_stream s) {
    const char* me = "ishara_op_bn_bwd_apply";
    OP_DT(me, dt, false);
    if (dwconv_bwd_refused(me, dt, B, T, C, 1, 0, {dy, h, mean, rstd, a, E, Fc, dx}, {"dy", "h", "mean", "rstd", "a", "E", "Fc", "dx"}, {sg})) return -1;
    return launch_bn_bwd_apply(dt, dy, h, mean, rstd, a, sg, E, e_per_sample ? 1 : 0, Fc, dx, B, T, C, (hipStream_t)s);
}
// the conv backward behind a BatchNorm, as convblock_bwd and the Conformer conv module's backward run it: the one-pass kernel with the
// BatchNorm backward folded into its row load where the route has one (returns 1), else ishara_op_bn_bwd_apply into tmp [B,T,C] (dt) and the
// plain backward on tmp (returns 0); < 0 on error.  sg and dbias may be NULL
extern "C" int ishara_op_dwconv_bwd_bn(int32_t dt, int32_t inop, const void* dy, const void* h, const float* mean, const float* rstd, const float* a, const float* sg,
                                       const float* E, int32_t e_per_sample, const float* Fc, const void* x, const float* w, void* dx, float* dw, float* dbias,
                                       void* scratch, void* tmp, int32_t B, int32_t T, int32_t C, int32_t k, int32_t padl, ishara_stream st) {
    const char* me = "ishara_op_dwconv_bwd_bn";
    OP_DT(me, dt, false);
    if (dwconv_bwd_refused(me, dt, B, T, C, k, padl, {dy, h, mean, rstd, a, E, Fc, x, w, dx, dw, tmp}, {"dy", "h", "mean", "rstd", "a", "E", "Fc", "x", "w", "dx", "dw", "tmp"},
                           {sg, dbias, scratch})) return -1;
    hipStream_t s = (hipStream_t)st;
    DwBnArgs bn; bn.h = h; bn.mean = mean; bn.rstd = rstd; bn.a = a; bn.sg = sg; bn.E = E; bn.Fc = Fc; bn.e_per_sample = e_per_sample ? 1 : 0;
    const int fused = launch_dwconv_bwd_bn(dt, inop, dy, bn, x, w, dx, dw, dbias, (float*)scratch, B, T, C, k, padl, s);
    if (fused != 0) return fused < 0 ? fused : 1;
    CK(launch_bn_bwd_apply(dt, dy, h, mean, rstd, a, sg, E, bn.e_per_sample, Fc, tmp, B, T, C, s));
    CK(launch_dwconv_bwd(dt, inop, tmp, x, w, dx, dw, dbias, (float*)scratch, B, T, C, k, padl, s));
    return 0;
}
// scratch layout: q | k | vt | lse | delta | maskw (q, k, vt sized for 4-byte elements whatever the dtype)
struct AttnScratch {
    void *q, *k, *vt; float *lse, *delta; uint32_t* maskw; size_t total;
    AttnScratch(char* sc, int B, int H, int T, int dh) {
        const size_t seg = rup((size_t)B * H * T * dh * 4, 256), row = rup((size_t)B * H * T * 4, 256);
        q = sc; k = sc + seg; vt = sc + 2 * seg;
        lse = (float*)(sc + 3 * seg);
        delta = (float*)(sc + 3 * seg + row);
        maskw = (uint32_t*)(sc + 3 * seg + 2 * row);
        total = 3 * seg + 2 * row + rup(attn_mask_words(B, H, T) * 4, 256);
    }
};
extern "C" int64_t ishara_op_attn_scratch_bytes(int32_t B, int32_t H, int32_t T, int32_t dh) { return (int64_t)AttnScratch(nullptr, B, H, T, dh).total; }
// where lse, delta and the keep-bit words lie inside that scratch: out[0..5] = byte offset and extent (bytes the kernels may write) of lse, of
// delta and of maskw.  Each region is rounded up to 256 bytes: what lies between an extent's end and the next offset (or the total) is padding
// that no kernel touches.  No handle, no HIP call.
extern "C" int ishara_op_attn_scratch_layout_bytes(int32_t B, int32_t H, int32_t T, int32_t dh, int64_t* out) {
    const char* me = "ishara_op_attn_scratch_layout_bytes";
    if (B < 1 || H < 1 || T < 1 || dh < 1) { ishara_set_error("%s: B=%d H=%d T=%d dh=%d: B, H, T and dh must be >= 1", me, B, H, T, dh); return -1; }
    if (!out) { ishara_set_error("%s: null out", me); return -1; }
    const AttnScratch a(nullptr, B, H, T, dh);
    const int64_t row = (int64_t)B * H * T * 4;
    out[0] = (int64_t)(uintptr_t)a.lse; out[1] = row;
    out[2] = (int64_t)(uintptr_t)a.delta; out[3] = row;
    out[4] = (int64_t)(uintptr_t)a.maskw; out[5] = (int64_t)attn_mask_words(B, H, T) * 4;
    return 0;
}
// impl: 0 lane-split, 1 MFMA with the keep bits cached in the scratch (DM 2), 2 MFMA with no keep-bit buffer: the backward kernels hash again
// (DM 1, the product's ISHARA_NO_ATTN_BITS route).  Everything a launch would fault or fail on is refused here, before any HIP call.
// Which kernel a call would run on is asked of attn_fwd_route / attn_bwd_route (attention.hip), as the launchers ask them.
static int attn_op_refused(const char* me, bool backward, int dt, int B, int H, int T, int dh, float rate, int impl, std::initializer_list<const void*> operands,
                           std::initializer_list<const char*> operand_names, const void* scratch) {
    if (B < 1 || H < 1 || T < 1) { ishara_set_error("%s: B=%d H=%d T=%d: B, H and T must be >= 1", me, B, H, T); return -1; }
    if (dh != 8 && dh != 16 && dh != 24 && dh != 32 && dh != 48 && dh != 64) { ishara_set_error("%s: head dim %d unsupported (8, 16, 24, 32, 48, 64)", me, dh); return -1; }
    if (impl < 0 || impl > 2) { ishara_set_error("%s: unknown impl %d (0 lane-split, 1 MFMA with cached keep bits, 2 MFMA hashing again in the backward)", me, impl); return -1; }
    const AttnRoute r = backward ? attn_bwd_route(dt, T, dh, impl >= 1, rate > 0.f, impl == 1, true) : attn_fwd_route(dt, T, dh, impl >= 1, rate > 0.f, impl == 1);
    const bool takes_bits = r.kind == ATT_MFMA || r.kind == ATT_BWD_TWO_KERNEL || r.kind == ATT_BWD_FUSED;      // a kernel that has the dropout modes 1 and 2
    if (impl == 2 && !takes_bits && r.kind != ATT_REFUSED) { ishara_set_error("%s: impl 2 has MFMA kernels only: ISHARA_BF16 and head dim 32 / 64 (dtype %d, head dim %d)", me, dt, dh); return -1; }
    // the caller checked the dtype (OP_DT) and the head dim passed above: what the route still refuses is a T the MFMA kernels do not take
    if (r.kind == ATT_REFUSED) { ishara_set_error("%s: T=%d: the MFMA kernels need T %% 8 == 0 (16-byte pieces of the V^T rows)", me, T); return -1; }
    if (!(rate >= 0.f && rate < 1.f)) { ishara_set_error("%s: rate %g outside [0, 1)", me, rate); return -1; }
    if ((int64_t)B * H > 65535 || (int64_t)B * H * T * dh * 3 > 2147483647LL) { ishara_set_error("%s: B=%d H=%d T=%d dh=%d: shape too large (B*H <= 65535: one grid row per head; 3*B*H*T*dh < 2^31)", me, B, H, T, dh); return -1; }
    for (size_t i = 0; i < operands.size(); ++i) if (!operands.begin()[i]) { ishara_set_error("%s: null %s", me, operand_names.begin()[i]); return -1; }
    if (!scratch) { ishara_set_error("%s: null scratch (ishara_op_attn_scratch_bytes)", me); return -1; }
    for (size_t i = 0; i < operands.size(); ++i)
        if ((uintptr_t)operands.begin()[i] % 16) { ishara_set_error("%s: misaligned %s: 16-byte aligned operands (vector loads and stores)", me, operand_names.begin()[i]); return -1; }
    if ((uintptr_t)scratch % 256) { ishara_set_error("%s: misaligned scratch: 256-byte aligned (the layout rounds every region to 256 bytes)", me); return -1; }
    return 0;
}
extern "C" int ishara_op_attn_fwd(int32_t dt, const void* qkv, void* o, int32_t B, int32_t H, int32_t T, int32_t dh, float scale,
                                  uint32_t seed, uint32_t site, float rate, int32_t impl, void* scratch, ishara_stream st) {
    OP_DT("ishara_op_attn_fwd", dt, true);
    if (dt == DT_F16 && rate > 0.f) { ishara_set_error("ishara_op_attn_fwd: ISHARA_F16 is inference-only: no attention dropout (rate %g)", rate); return -1; }
    if (attn_op_refused("ishara_op_attn_fwd", false, dt, B, H, T, dh, rate, impl, {qkv, o}, {"qkv", "o"}, scratch)) return -1;
    hipStream_t s = (hipStream_t)st;
    const AttnScratch a((char*)scratch, B, H, T, dh);
    if (dt == DT_BF16) hipLaunchKernelGGL(qkv_split_kernel<bf16>, dim3(1024), dim3(256), 0, s, (const bf16*)qkv, (bf16*)a.q, (bf16*)a.k, (bf16*)a.vt, B, H, T, dh);
    else if (dt == DT_F16) hipLaunchKernelGGL(qkv_split_kernel<f16>, dim3(1024), dim3(256), 0, s, (const f16*)qkv, (f16*)a.q, (f16*)a.k, (f16*)a.vt, B, H, T, dh);
    else hipLaunchKernelGGL(qkv_split_kernel<float>, dim3(1024), dim3(256), 0, s, (const float*)qkv, (float*)a.q, (float*)a.k, (float*)a.vt, B, H, T, dh);
    return launch_attn_fwd(dt, a.q, a.k, a.vt, o, a.lse, B, H, T, dh, scale, make_drop_attn(seed, site, rate, true), impl == 2 ? 1 : impl, impl == 2 ? nullptr : a.maskw, s);
}
extern "C" int ishara_op_attn_bwd(int32_t dt, const void* o, const void* dout, void* dqkv, int32_t B, int32_t H, int32_t T, int32_t dh, float scale,
                                  uint32_t seed, uint32_t site, float rate, int32_t impl, void* scratch, ishara_stream st) {
    OP_DT("ishara_op_attn_bwd", dt, false);
    if (attn_op_refused("ishara_op_attn_bwd", true, dt, B, H, T, dh, rate, impl, {o, dout, dqkv}, {"o", "dout", "dqkv"}, scratch)) return -1;
    hipStream_t s = (hipStream_t)st;
    const AttnScratch a((char*)scratch, B, H, T, dh);
    return launch_attn_bwd(dt, a.q, a.k, a.vt, o, dout, a.lse, a.delta, dqkv, B, H, T, dh, scale, make_drop_attn(seed, site, rate, true), 1, impl == 2 ? 1 : impl,
                           impl == 2 ? nullptr : a.maskw, s);
}

// ---- operator tests: the torch Squeezeformer family's own kernels (r4_subsample.hip, relattn_len.hip), through the launch code the encoder uses.
// The family has no fp16 kernels: every entry point refuses ISHARA_F16.  Shapes, null and alignment are checked before any HIP call;
// every output, the parameter gradients included, is overwritten.
static bool op_r4_dt_ok(const char* op, int dt) {
    if (dt != DT_F32 && dt != DT_BF16 && dt != DT_F16) { ishara_set_error("%s: unknown dtype %d (ISHARA_F32 = 0, ISHARA_BF16 = 1, ISHARA_F16 = 2)", op, dt); return false; }
    if (dt == DT_F16) { ishara_set_error("%s: ISHARA_F16 is not supported (the torch Squeezeformer family has no fp16 kernels)", op); return false; }
    return true;
}
#define OP_R4_DT(op, dt) do { if (!op_r4_dt_ok(op, dt)) return -1; } while (0)
static bool op_misaligned(std::initializer_list<const void*> ps) { uintptr_t a = 0; for (const void* p : ps) a |= (uintptr_t)p; return a % 16 != 0; }
static bool op_any_null(std::initializer_list<const void*> ps) { for (const void* p : ps) if (!p) return true; return false; }
static size_t op_shadow_bytes(int K, int N, int M) { const size_t a = OpShadow(DT_F32, K, N, M).total, b = OpShadow(DT_BF16, K, N, M).total; return rup(a > b ? a : b, 256); }

// scratch of the relative attention: pos_proj shadows and wgrad slab | table in the storage dtype | posp | dposp | lse | delta
struct RelAttnScratch {
    size_t pedt, posp, dposp, lse, delta, total;
    RelAttnScratch(int B, int H, int T, int dh) {
        const size_t d = (size_t)H * dh, R = 2 * (size_t)T - 1, tab = rup(R * d * 4, 256), row = rup((size_t)B * H * T * 4, 256);
        pedt = op_shadow_bytes((int)d, (int)d, (int)R);
        posp = pedt + tab; dposp = posp + tab; lse = dposp + tab; delta = lse + row; total = delta + row;
    }
};
static const char* relattn_shape_error(int B, int H, int T, int dh, float rate) {
    if (!relattn_head_dim_ok(dh)) return "head dim unsupported (" RELATTN_HEAD_DIMS ")";
    if (B < 1 || H < 1 || T < 1) return "B, H and T must be >= 1";
    if ((int64_t)B * H > 65535 || (int64_t)B * H * T * dh > 2147483647LL || (2 * (int64_t)T - 1) * H * dh > 2147483647LL) return "shape too large (B*H <= 65535, B*H*T*dh < 2^31)";
    if (!(rate >= 0.f && rate < 1.f)) return "rate outside [0, 1)";
    return nullptr;
}
extern "C" int64_t ishara_op_relattn_scratch_bytes(int32_t B, int32_t H, int32_t T, int32_t dh) {
    if (relattn_shape_error(B, H, T, dh, 0.f)) return -1;
    return (int64_t)RelAttnScratch(B, H, T, dh).total;
}
// ---- the two pairs of entry points, one body each.  ishara_op_relattn_fwd / _bwd: no lengths (key_len NULL: every key).  ishara_relattn_len_fwd /
// _bwd: key_len device int32 [B], the keys j >= clamp(key_len[b], 0, T) of clip b are masked for every query and head; route: 0 the plan's
// choice (relattn_route), 1 the fp32 lane kernels.  The checks and messages are the same, then key_len and route where lengths are taken.
// The second pair is named outside the ishara_op_ prefix: it takes key lengths, which no other operator entry point does
static int relattn_len_refused(const char* me, const int32_t* key_len, int32_t route) {
    if (!key_len || (uintptr_t)key_len % 4) { ishara_set_error("%s: null or misaligned key_len: an int32 array [B]", me); return -1; }
    if (route != 0 && route != 1) { ishara_set_error("%s: route %d unknown (0 the plan's choice, 1 the fp32 lane kernels)", me, route); return -1; }
    return 0;
}
static int relattn_fwd_op(const char* me, bool lengths, int32_t dt, const void* q, const void* k, const void* v, const float* pe, const float* Wpos, const float* u, const float* vb,
                          void* o, float* lse, int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate,
                          const int32_t* key_len, int32_t route, void* scratch, ishara_stream st) {
    OP_R4_DT(me, dt);
    if (const char* why = relattn_shape_error(B, H, T, dh, rate)) { ishara_set_error("%s: B=%d H=%d T=%d dh=%d rate=%g: %s", me, B, H, T, dh, rate, why); return -1; }
    if (op_any_null({q, k, v, pe, Wpos, u, vb, o, scratch}) || op_misaligned({q, k, v, pe, Wpos, u, vb, o, lse, scratch})) {
        ishara_set_error("%s: null or misaligned buffer (all 16-byte aligned; only lse may be NULL)", me); return -1;
    }
    if (lengths && relattn_len_refused(me, key_len, route)) return -1;
    hipStream_t s = (hipStream_t)st;
    const int d = H * dh, R = 2 * T - 1;
    const OpShadow sh(dt, d, d, R);
    const RelAttnScratch a(B, H, T, dh);
    char* sc = (char*)scratch;
    CK(sh.build(dt, Wpos, d, d, sc, s));
    // the table in the storage type (A operand of the pos_proj GEMM), as r4_forward converts it
    if (dt != DT_F32) CK(r5_from_f32(dt, pe, sc + a.pedt, (size_t)R * d, s));
    else HIP_CHECK_RET(hipMemcpyAsync(sc + a.pedt, pe, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    OpArgs no; EpiArgs e0;
    CK(launch_gemm_nt(dt, dt, DT_F32, OP_NONE, sc + a.pedt, sc + sh.wt, sc + a.posp, R, d, d, sh.ldt, no, e0, s));      // r4_mhsa_fwd's pos_proj
    CK(launch_relattn_len_fwd(dt, q, k, v, (const float*)(sc + a.posp), u, vb, o, (float*)(sc + a.lse), key_len, route == 1, B, H, T, dh, 1.0f / sqrtf((float)dh),
                              make_drop_attn(seed, site, rate, true), s));
    if (lse) HIP_CHECK_RET(hipMemcpyAsync(lse, sc + a.lse, (size_t)B * H * T * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
static int relattn_bwd_op(const char* me, bool lengths, int32_t dt, const void* q, const void* k, const void* v, const float* u, const float* vb, const void* o, const void* dO,
                          void* dq, void* dk, void* dv, float* du, float* dvb, float* dWpos, float* dposp,
                          int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate,
                          const int32_t* key_len, int32_t route, void* scratch, ishara_stream st) {
    OP_R4_DT(me, dt);
    if (const char* why = relattn_shape_error(B, H, T, dh, rate)) { ishara_set_error("%s: B=%d H=%d T=%d dh=%d rate=%g: %s", me, B, H, T, dh, rate, why); return -1; }
    if (op_any_null({q, k, v, u, vb, o, dO, dq, dk, dv, du, dvb, dWpos, scratch}) || op_misaligned({q, k, v, u, vb, o, dO, dq, dk, dv, du, dvb, dWpos, dposp, scratch})) {
        ishara_set_error("%s: null or misaligned buffer (all 16-byte aligned; only dposp may be NULL)", me); return -1;
    }
    if (lengths && relattn_len_refused(me, key_len, route)) return -1;
    hipStream_t s = (hipStream_t)st;
    const int d = H * dh, R = 2 * T - 1;
    const OpShadow sh(dt, d, d, R);
    const RelAttnScratch a(B, H, T, dh);
    char* sc = (char*)scratch;
    float* dp = (float*)(sc + a.dposp);
    CK(r4_fill_f32_launch(dp, (size_t)R * d, 0.f, s));
    CK(r4_fill_f32_launch(du, (size_t)d, 0.f, s));
    CK(r4_fill_f32_launch(dvb, (size_t)d, 0.f, s));
    CK(r4_fill_f32_launch(dWpos, (size_t)d * d, 0.f, s));
    CK(launch_relattn_len_bwd(dt, q, k, v, (const float*)(sc + a.posp), u, vb, o, dO, (const float*)(sc + a.lse), (float*)(sc + a.delta), dq, dk, dv, du, dvb, dp,
                              key_len, B, H, T, dh, 1.0f / sqrtf((float)dh), make_drop_attn(seed, site, rate, true), s));      // the route's one backward
    OpArgs no;
    CK(launch_gemm_tn(dt, DT_F32, dt, OP_NONE, OP_NONE, sc + a.pedt, dp, dWpos, nullptr, (float*)(sc + sh.slab), R, d, d, no, no, s));      // r4_mhsa_bwd's pos_proj weight gradient
    if (dposp) HIP_CHECK_RET(hipMemcpyAsync(dposp, dp, (size_t)R * d * sizeof(float), hipMemcpyDeviceToDevice, s));
    return 0;
}
extern "C" int ishara_op_relattn_fwd(int32_t dt, const void* q, const void* k, const void* v, const float* pe, const float* Wpos, const float* u, const float* vb,
                                     void* o, float* lse, int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate, void* scratch, ishara_stream st) {
    return relattn_fwd_op("ishara_op_relattn_fwd", false, dt, q, k, v, pe, Wpos, u, vb, o, lse, B, H, T, dh, seed, site, rate, nullptr, 0, scratch, st);
}
extern "C" int ishara_op_relattn_bwd(int32_t dt, const void* q, const void* k, const void* v, const float* u, const float* vb, const void* o, const void* dO,
                                     void* dq, void* dk, void* dv, float* du, float* dvb, float* dWpos, float* dposp,
                                     int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate, void* scratch, ishara_stream st) {
    return relattn_bwd_op("ishara_op_relattn_bwd", false, dt, q, k, v, u, vb, o, dO, dq, dk, dv, du, dvb, dWpos, dposp, B, H, T, dh, seed, site, rate, nullptr, 0, scratch, st);
}
extern "C" int64_t ishara_relattn_len_scratch_bytes(int32_t B, int32_t H, int32_t T, int32_t dh) { return ishara_op_relattn_scratch_bytes(B, H, T, dh); }
extern "C" const char* ishara_debug_relattn_kernel_name(int32_t dt, int32_t backward, int32_t T, int32_t dh, int32_t masked) {
    return relattn_kernel_name(relattn_route(dt, T, dh, masked != 0), backward != 0);
}
extern "C" int ishara_relattn_len_fwd(int32_t dt, const void* q, const void* k, const void* v, const float* pe, const float* Wpos, const float* u, const float* vb,
                                      void* o, float* lse, int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate,
                                      const int32_t* key_len, int32_t route, void* scratch, ishara_stream st) {
    return relattn_fwd_op("ishara_relattn_len_fwd", true, dt, q, k, v, pe, Wpos, u, vb, o, lse, B, H, T, dh, seed, site, rate, key_len, route, scratch, st);
}
extern "C" int ishara_relattn_len_bwd(int32_t dt, const void* q, const void* k, const void* v, const float* u, const float* vb, const void* o, const void* dO,
                                      void* dq, void* dk, void* dv, float* du, float* dvb, float* dWpos, float* dposp,
                                      int32_t B, int32_t H, int32_t T, int32_t dh, uint32_t seed, uint32_t site, float rate,
                                      const int32_t* key_len, int32_t route, void* scratch, ishara_stream st) {
    return relattn_bwd_op("ishara_relattn_len_bwd", true, dt, q, k, v, u, vb, o, dO, dq, dk, dv, du, dvb, dWpos, dposp, B, H, T, dh, seed, site, rate, key_len, route, scratch, st);
}

// DepthwiseConv2dSubsampling.  scratch: y1 | dz1, both [B, d, T1, F1] f32
static const char* subsample_shape_error(int B, int T0, int F, int d) {
    if (B < 1 || d < 1) return "B and d must be >= 1";
    if (T0 < 7 || F < 7) return "T0 and F must be >= 7 (two 3x3 stride-2 convolutions)";
    const R4Dims D = r4_dims(T0, F, d);
    if ((int64_t)B * d * D.T1 * D.F1 > 2147483647LL || (int64_t)B * T0 * F > 2147483647LL) return "shape too large (B*d*T1*F1 < 2^31)";
    return nullptr;
}
extern "C" int64_t ishara_op_r4_subsample_scratch_bytes(int32_t B, int32_t T0, int32_t F, int32_t d) {
    if (subsample_shape_error(B, T0, F, d)) return -1;
    const R4Dims D = r4_dims(T0, F, d);
    return (int64_t)(2 * rup((size_t)B * d * D.T1 * D.F1 * 4, 256));
}
extern "C" int ishara_op_r4_subsample_fwd(int32_t dt, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, void* sub,
                                          int32_t B, int32_t T0, int32_t F, int32_t d, void* scratch, ishara_stream st) {
    const char* me = "ishara_op_r4_subsample_fwd";
    OP_R4_DT(me, dt);
    if (const char* why = subsample_shape_error(B, T0, F, d)) { ishara_set_error("%s: B=%d T0=%d F=%d d=%d: %s", me, B, T0, F, d, why); return -1; }
    if (op_any_null({x, w1, b1, w2, b2, sub, scratch}) || op_misaligned({x, w1, b1, w2, b2, sub, scratch})) { ishara_set_error("%s: null or misaligned buffer (all 16-byte aligned)", me); return -1; }
    const R4Dims D = r4_dims(T0, F, d);
    return r4_subsample_fwd_launch(dt, x, w1, b1, w2, b2, (float*)scratch, sub, B, T0, F, d, D.T1, D.F1, D.T2, D.F2, (hipStream_t)st);
}
extern "C" int ishara_op_r4_subsample_bwd(int32_t dt, const float* x, const float* w1, const float* w2, const void* sub, const void* dsub,
                                          float* dw1, float* db1, float* dw2, float* db2, float* dx, int32_t B, int32_t T0, int32_t F, int32_t d, void* scratch, ishara_stream st) {
    const char* me = "ishara_op_r4_subsample_bwd";
    OP_R4_DT(me, dt);
    if (const char* why = subsample_shape_error(B, T0, F, d)) { ishara_set_error("%s: B=%d T0=%d F=%d d=%d: %s", me, B, T0, F, d, why); return -1; }
    if (op_any_null({x, w1, w2, sub, dsub, dw1, db1, dw2, db2, scratch}) || op_misaligned({x, w1, w2, sub, dsub, dw1, db1, dw2, db2, dx, scratch})) {
        ishara_set_error("%s: null or misaligned buffer (all 16-byte aligned; only dx may be NULL)", me); return -1;
    }
    hipStream_t s = (hipStream_t)st;
    const R4Dims D = r4_dims(T0, F, d);
    float* y1 = (float*)scratch;
    float* dz1 = (float*)((char*)scratch + rup((size_t)B * d * D.T1 * D.F1 * 4, 256));
    CK(r4_fill_f32_launch(dw1, (size_t)d * 9, 0.f, s)); CK(r4_fill_f32_launch(db1, (size_t)d, 0.f, s));
    CK(r4_fill_f32_launch(dw2, (size_t)d * 9, 0.f, s)); CK(r4_fill_f32_launch(db2, (size_t)d, 0.f, s));
    return r4_subsample_bwd_launch(dt, dsub, sub, y1, x, w1, w2, dz1, dw1, db1, dw2, db2, dx, B, T0, F, d, D.T1, D.F1, D.T2, D.F2, s);
}

// TimeReductionLayer + time_reduction_proj.  scratch: the Linear's shadows ([Fr, d], K zero-padded to Kp) | wgrad slab | pre | conv output
// [B*Tr, Kp] | its gradient | the [Kp, d] weight-gradient scratch
struct TredScratch {
    int Tr, Fr, Kp, M; size_t slab, pre, trout, dtrout, dwred, total;
    TredScratch(int B, int Tin, int d) {
        Tr = (Tin - 3) / 2 + 1; Fr = (d - 1) / 2; Kp = (int)rup(Fr, 8); M = B * Tr;
        const OpShadow f(DT_F32, Fr, d, M), h(DT_BF16, Fr, d, M);
        slab = rup(f.slab > h.slab ? f.slab : h.slab, 256);
        const size_t sf = gemm_tn_slab_floats(M, Kp, d, DT_F32), sh = gemm_tn_slab_floats(M, Kp, d, DT_BF16);
        pre = slab + rup((sf > sh ? sf : sh) * 4, 256);
        trout = pre + rup((size_t)M * Fr * 4, 256);
        dtrout = trout + rup((size_t)M * Kp * 4, 256);
        dwred = dtrout + rup((size_t)M * Kp * 4, 256);
        total = dwred + rup((size_t)Kp * d * 4, 256);
    }
};
static const char* tred_shape_error(int B, int Tin, int d) {
    if (B < 1) return "B must be >= 1";
    if (Tin < 3 || d < 3) return "Tin and d must be >= 3 (one 3x3 stride-2 convolution)";
    if (d % 8 != 0) return "d must be a multiple of 8 (16-byte rows of the Linear)";
    if ((int64_t)B * Tin * d > 2147483647LL) return "shape too large (B*Tin*d < 2^31)";
    return nullptr;
}
extern "C" int64_t ishara_op_r4_time_reduce_scratch_bytes(int32_t B, int32_t Tin, int32_t d) {
    if (tred_shape_error(B, Tin, d)) return -1;
    return (int64_t)TredScratch(B, Tin, d).total;
}
extern "C" int ishara_op_r4_time_reduce_fwd(int32_t dt, const void* h, const float* conv_w, const float* conv_b, const float* Wred, const float* bred, void* red, void* conv_out,
                                            int32_t B, int32_t Tin, int32_t d, void* scratch, ishara_stream st) {
    const char* me = "ishara_op_r4_time_reduce_fwd";
    OP_R4_DT(me, dt);
    if (const char* why = tred_shape_error(B, Tin, d)) { ishara_set_error("%s: B=%d Tin=%d d=%d: %s", me, B, Tin, d, why); return -1; }
    if (op_any_null({h, conv_w, conv_b, Wred, bred, red, scratch}) || op_misaligned({h, conv_w, conv_b, Wred, bred, red, conv_out, scratch})) {
        ishara_set_error("%s: null or misaligned buffer (all 16-byte aligned; only conv_out may be NULL)", me); return -1;
    }
    hipStream_t s = (hipStream_t)st;
    const TredScratch a(B, Tin, d);
    const OpShadow sh(dt, a.Fr, d, a.M);
    char* sc = (char*)scratch;
    CK(sh.build(dt, Wred, a.Fr, d, sc, s));
    CK(r4_tred_fwd_launch(dt, h, conv_w, conv_b, (float*)(sc + a.pre), sc + a.trout, B, Tin, d, a.Tr, a.Fr, a.Kp, s));
    OpArgs no; EpiArgs ea; ea.bias = bred;
    CK(launch_gemm_nt(dt, dt, dt, OP_NONE, sc + a.trout, sc + sh.wt, red, a.M, d, a.Kp, sh.ldt, no, ea, s));      // r4_forward's Linear over K = Kp
    if (conv_out) HIP_CHECK_RET(hipMemcpyAsync(conv_out, sc + a.trout, (size_t)a.M * a.Kp * dt_size(dt), hipMemcpyDeviceToDevice, s));
    return 0;
}
extern "C" int ishara_op_r4_time_reduce_bwd(int32_t dt, const void* h, const float* conv_w, const void* dred, const void* extra, void* dh,
                                            float* dconv_w, float* dconv_b, float* dWred, float* dbred, int32_t B, int32_t Tin, int32_t d, void* scratch, ishara_stream st) {
    const char* me = "ishara_op_r4_time_reduce_bwd";
    OP_R4_DT(me, dt);
    if (const char* why = tred_shape_error(B, Tin, d)) { ishara_set_error("%s: B=%d Tin=%d d=%d: %s", me, B, Tin, d, why); return -1; }
    if (op_any_null({h, conv_w, dred, dh, dconv_w, dconv_b, dWred, dbred, scratch}) || op_misaligned({h, conv_w, dred, extra, dh, dconv_w, dconv_b, dWred, dbred, scratch})) {
        ishara_set_error("%s: null or misaligned buffer (all 16-byte aligned; only extra may be NULL)", me); return -1;
    }
    hipStream_t s = (hipStream_t)st;
    const TredScratch a(B, Tin, d);
    const OpShadow sh(dt, a.Fr, d, a.M);
    char* sc = (char*)scratch;
    OpArgs no; EpiArgs e0;
    CK(launch_gemm_nt(dt, dt, dt, OP_NONE, dred, sc + sh.wn, sc + a.dtrout, a.M, a.Kp, d, sh.ldn, no, e0, s));      // r4_backward's dgrad: d conv output [B*Tr, Kp]
    CK(r4_fill_f32_launch(dWred, (size_t)a.Fr * d, 0.f, s)); CK(r4_fill_f32_launch(dbred, (size_t)d, 0.f, s));
    CK(r4_fill_f32_launch(dconv_w, 9, 0.f, s)); CK(r4_fill_f32_launch(dconv_b, 1, 0.f, s));
    CK(r4_tred_wgrad_launch(dt, sc + a.trout, dred, (float*)(sc + a.dwred), dWred, dbred, (float*)(sc + a.slab), a.M, a.Fr, a.Kp, d, s));
    return r4_tred_bwd_launch(dt, sc + a.dtrout, (const float*)(sc + a.pre), h, conv_w, extra, dconv_w, dconv_b, dh, B, Tin, d, a.Tr, a.Fr, a.Kp, s);
}

// the row maps r4_rows<MODE> over [B, Tdst, d]: 0 dst[t] = src[t/2]; 1 dst[t] = src[t] (crop); 2 dst[t] = src[2t] + src[2t+1]; 3 dst[t] = t < Tsrc ? src[t] : 0; 4 dst = a + src
extern "C" int ishara_op_r4_rows(int32_t dt, int32_t mode, const void* src, const void* a, void* dst, int32_t B, int32_t Tdst, int32_t Tsrc, int32_t d, ishara_stream st) {
    const char* me = "ishara_op_r4_rows";
    OP_R4_DT(me, dt);
    if (mode < 0 || mode > 4) { ishara_set_error("%s: unknown mode %d (0..4)", me, mode); return -1; }
    if (B < 1 || Tdst < 1 || Tsrc < 1 || d < 1 || (int64_t)B * (Tdst > Tsrc ? Tdst : Tsrc) * d > 2147483647LL) { ishara_set_error("%s: bad shape B=%d Tdst=%d Tsrc=%d d=%d", me, B, Tdst, Tsrc, d); return -1; }
    if ((mode == 0 && Tdst > 2 * Tsrc) || (mode == 1 && Tdst > Tsrc) || (mode == 2 && 2 * Tdst > Tsrc) || (mode == 4 && Tdst != Tsrc)) {
        ishara_set_error("%s: mode %d reads past the source rows (Tdst=%d Tsrc=%d)", me, mode, Tdst, Tsrc); return -1;
    }
    if (!src || !dst || (mode == 4 && !a) || op_misaligned({src, a, dst})) { ishara_set_error("%s: null or misaligned buffer (16-byte aligned; a is read by mode 4 only)", me); return -1; }
    return r4_rows_mode_launch(dt, mode, src, a, dst, B, Tdst, Tsrc, d, (hipStream_t)st);
}
