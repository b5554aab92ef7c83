// Host side of libishara_hip.so that every model family shares: the handle's life cycle (create / bind / weight shadows / gradient
// buckets / optimizer / profiler) and the plumbing the families' graphs are written with (parameter layout, workspace plan helpers,
// profiled GEMM wrappers, deferred parameter-gradient sums).  The families themselves: keras_graph.hip / conv_block.hip / keras_hybrid.hip / keras_probe.hip, conformer_r5.hip,
// squeezeformer_r4.hip; the stand-alone and operator entry points: api_ops.hip.  Everything is launched on the caller's stream.
#include "model_types.h"
#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <utility>
#include <stdlib.h>

// ------------------------------------------------------------------ error string
static thread_local char g_err[1024] = "";
void ishara_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* ishara_last_error(void) { return g_err; }

// ------------------------------------------------------------------ small kernels
// fills inside forward / backward use a kernel rather than hipMemsetAsync, so that a captured forward / training step holds kernel
// nodes only.  (Round 1 blamed hipGraph memset nodes for intermittently wrong replays; round 2 could not reproduce that — 0 of 72 000
// checks wrong with memset nodes, profiles/r2_graph_memset_experiment.txt — and withdrew the attribution: DESIGN.md §4.)
__global__ void fill_u32_kernel(uint32_t* p, size_t n, uint32_t v) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}
int launch_fill_u32(void* p, size_t n_words, uint32_t v, hipStream_t s) {
    if (n_words == 0) return 0;
    const int grid = (int)((n_words + 255) / 256 < 1024 ? (n_words + 255) / 256 : 1024);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(grid), dim3(256), 0, s, (uint32_t*)p, n_words, v);
    return launch_rc();
}

// ------------------------------------------------------------------ construction helpers of the three families
// physical offsets: trainable first, then BatchNorm moving statistics
void finish_param_layout(ishara_model* m) {
    int64_t off = 0;
    for (auto& e : m->entries) if (e.trainable) { e.offset = off; off += e.shape[0] * (e.ndim == 2 ? e.shape[1] : 1); }
    m->n_train = off;
    for (auto& e : m->entries) if (!e.trainable) { e.offset = off; off += e.shape[0] * (e.ndim == 2 ? e.shape[1] : 1); }
    m->n_total = off;
}

void plan_shadow(ishara_model* m, DenseW& w, int min_ldt, int min_ldn) {
    const size_t es = dt_size(m->dt);
    w.ldt = shadow_ld(m->dt, w.K, min_ldt);      // zero-padded K (the shadow arena is zero-filled, the builder writes k < K)
    w.wt = m->alloc(rup(w.N, 128) * (size_t)w.ldt * es).off;
    w.ldn = shadow_ld(m->dt, w.N, min_ldn);
    w.wn = m->alloc(rup(w.K, 128) * (size_t)w.ldn * es).off;
    m->denses.push_back(&w);
}
// activations of a ConfConv / a post-LN FFN over `rows` = Bmax * T rows of that layer (allocation order is the workspace layout)
void plan_confconv(ishara_model* m, ConfConv& c, size_t rows, int B, int d) {
    auto A = [&](int cols) { return m->alloc(rows * cols * dt_size(m->dt)); };
    c.g = A(2 * d); c.v = A(d); c.bnv = A(d);
    if (c.swish_after_bn) c.sw = A(d);
    c.ssum = m->f32((size_t)B * d); c.ssq = m->f32((size_t)B * d);
    c.mean = m->f32(d); c.rstd = m->f32(d); c.a = m->f32(d); c.bsh = m->f32(d);
    c.r = A(d); c.lnmean = m->f32(rows); c.lnrstd = m->f32(rows); c.out = A(d);
}
void plan_post_ln_ffn(ishara_model* m, R5FFN& f, size_t rows, int d, int de) {
    auto A = [&](int cols) { return m->alloc(rows * cols * dt_size(m->dt)); };
    f.za = A(de); f.u = A(de); f.r = A(d); f.mean = m->f32(rows); f.rstd = m->f32(rows); f.out = A(d);
}
// floats of the split-M partial sums of the largest weight-gradient GEMM over M rows: every planned Dense (its K at least min_K) and the
// packed stem operand where the model has one
size_t wgrad_slab_floats(const ishara_model* m, size_t M, int min_K) {
    size_t slabf = 0;
    for (const DenseW* w : m->denses) { const size_t f = gemm_tn_slab_floats((int)M, w->K > min_K ? w->K : min_K, w->N, m->dt); if (f > slabf) slabf = f; }
    if (m->stem_kp) { const size_t f = gemm_tn_slab_floats((int)M, m->stem_kp, m->d, m->dt); if (f > slabf) slabf = f; }
    return slabf;
}
// floats of the shared slab: those, the LayerNorm backward and the depthwise conv forward / backward over up to 2 * maxw channels
size_t slab_floats(const ishara_model* m, size_t M, int B, int T, int maxw, int min_K) {
    size_t slabf = wgrad_slab_floats(m, M, min_K);
    if (layernorm_bwd_scratch_floats(m->d) > slabf) slabf = layernorm_bwd_scratch_floats(m->d);
    if (dwconv_bwd_scratch_floats(2 * maxw, 31) > slabf) slabf = dwconv_bwd_scratch_floats(2 * maxw, 31);
    if (dwconv_fwd_scratch_floats(B, T, 2 * maxw) > slabf) slabf = dwconv_fwd_scratch_floats(B, T, 2 * maxw);
    return slabf;
}

static ishara_model* new_handle(const ishara_config& c, int C, int dtop, int L) {
    ishara_model* m = new ishara_model();
    m->cfg = c; m->dt = c.dtype == ISHARA_BF16 ? DT_BF16 : (c.dtype == ISHARA_F16 ? DT_F16 : DT_F32);
    m->d = c.dim; m->T = c.frames; m->F = c.features; m->C = C; m->H = c.num_heads; m->dh = c.dim / c.num_heads;
    m->dtop = dtop; m->Bmax = c.max_batch; m->L = L;
    m->family = c.family;
    { const char* gv = getenv("ISHARA_WS_GUARD"); m->guard = gv && gv[0] == '1'; }
    return m;
}

extern "C" int ishara_create(const ishara_config* cfg, ishara_model** out) {
    if (!cfg || !out) { ishara_set_error("ishara_create: null argument"); return -1; }
    ishara_config c = *cfg;
    if (c.family != ISHARA_FAMILY_KERAS_HYBRID && c.family != ISHARA_FAMILY_TORCH_CONFORMER && c.family != ISHARA_FAMILY_TORCH_SQUEEZEFORMER) { ishara_set_error("family=%d unknown", c.family); return -1; }
    if (c.family == ISHARA_FAMILY_TORCH_SQUEEZEFORMER) {    // squeezeformer/encoder.py: its own front end (conv2d subsampling), no head, no CTC; any frame count
        CK(r4_validate(c));
        if (c.dim <= 0 || c.dim % 8 != 0 || c.dim > 512 || c.num_heads <= 0 || c.dim % c.num_heads != 0) { ishara_set_error("encoder_dim=%d / heads=%d unsupported", c.dim, c.num_heads); return -1; }
        if (c.transformer_kernel_size < 1 || c.transformer_kernel_size > 31 || c.transformer_kernel_size % 2 == 0) { ishara_set_error("conv_kernel_size must be odd, 1..31"); return -1; }
        if (c.max_batch <= 0 || (c.dtype != ISHARA_F32 && c.dtype != ISHARA_BF16)) { ishara_set_error("max_batch / dtype unsupported"); return -1; }
        ishara_model* m = new_handle(c, 60, 2 * c.dim, 64);
        r4_build_graph(m); r4_plan_workspace(m);
        *out = m;
        return 0;
    }
    if (c.family == ISHARA_FAMILY_TORCH_CONFORMER) {      // conformer/conformer.py: no stem, no head, no CTC — the encoder stack only
        CK(r5_validate(c));
        c.features = c.dim; c.num_conv_per_block = 0; c.num_conv_squeeze_blocks = 0;
        if (c.num_classes <= 0) c.num_classes = 60;
        if (c.num_kernel_sizes <= 0) { c.num_kernel_sizes = 1; c.kernel_sizes[0] = 3; }
    }
    if (c.dim <= 0 || c.dim % 8 != 0 || c.dim > 512) { ishara_set_error("dim=%d unsupported (multiple of 8, <=512)", c.dim); return -1; }
    if (c.num_heads <= 0 || c.dim % c.num_heads != 0) { ishara_set_error("dim %% num_heads != 0"); return -1; }
    const int dh = c.dim / c.num_heads;
    if (dh != 8 && dh != 16 && dh != 24 && dh != 32 && dh != 48 && dh != 64) { ishara_set_error("head dim %d unsupported (8,16,24,32,48,64)", dh); return -1; }
    if (c.frames <= 0 || c.frames % 8 != 0 || c.frames > 512) { ishara_set_error("frames=%d unsupported (multiple of 8, <=512)", c.frames); return -1; }
    if (c.features <= 0 || c.features % 4 != 0) { ishara_set_error("features=%d unsupported (positive multiple of 4: 16-byte input rows)", c.features); return -1; }
    if (c.num_classes < 2 || c.num_classes > 64) { ishara_set_error("num_classes=%d unsupported (2..64)", c.num_classes); return -1; }
    if (c.num_kernel_sizes <= 0 && c.num_conv_per_block > 0) { ishara_set_error("kernel_sizes is empty"); return -1; }
    if (c.num_kernel_sizes > 8) { ishara_set_error("at most 8 kernel sizes"); return -1; }
    for (int i = 0; i < c.num_kernel_sizes; ++i) if (c.kernel_sizes[i] < 1 || c.kernel_sizes[i] > 31) { ishara_set_error("kernel size %d unsupported (1..31)", c.kernel_sizes[i]); return -1; }
    if (c.transformer_kernel_size < 1 || c.transformer_kernel_size > 31 || c.transformer_kernel_size % 2 == 0) { ishara_set_error("transformer_kernel_size must be odd, 1..31"); return -1; }
    if (c.max_batch <= 0) { ishara_set_error("max_batch must be > 0"); return -1; }
    if (c.dtype != ISHARA_F32 && c.dtype != ISHARA_BF16 && c.dtype != ISHARA_F16) { ishara_set_error("dtype must be ISHARA_F32, ISHARA_BF16 or ISHARA_F16"); return -1; }
    if (c.dtype == ISHARA_F16 && c.family != ISHARA_FAMILY_KERAS_HYBRID) { ishara_set_error("ISHARA_F16 (inference-only storage) exists for the Keras hybrid family only"); return -1; }
    if (c.top_dim <= 0) c.top_dim = 2 * c.dim;
    if (c.top_dim % 8 != 0) { ishara_set_error("top_dim must be a multiple of 8"); return -1; }
    if (c.max_label_len <= 0) c.max_label_len = 64;
    if (c.max_label_len > 255) { ishara_set_error("max_label_len > 255"); return -1; }
    ishara_model* m = new_handle(c, c.num_classes, c.top_dim, c.max_label_len);
    if (m->family == ISHARA_FAMILY_TORCH_CONFORMER) { r5_build_graph(m); r5_plan_workspace(m); *out = m; return 0; }
    keras_build_graph(m);
    keras_plan_workspace(m);
    // positional encoding table (c5:226-235): [sin | cos] halves, fp32 arithmetic
    m->pe_host.resize((size_t)m->T * m->d);
    const int half = m->d / 2;
    for (int t = 0; t < m->T; ++t)
        for (int i = 0; i < half; ++i) {
            const float depth = (float)i / (float)half;
            const float rate = 1.0f / powf(10000.0f, depth);
            const float ang = (float)t * rate;
            m->pe_host[(size_t)t * m->d + i] = sinf(ang);
            m->pe_host[(size_t)t * m->d + half + i] = cosf(ang);
        }
    *out = m;
    return 0;
}
extern "C" void ishara_destroy(ishara_model* m) {
    if (m) for (auto e : m->bucket_ev) (void)hipEventDestroy(e);
    if (m && m->r4) r4_destroy(m);
    delete m;
}
extern "C" int64_t ishara_param_total(const ishara_model* m) { return m->n_total; }
extern "C" int64_t ishara_param_trainable(const ishara_model* m) { return m->n_train; }
extern "C" int32_t ishara_param_entries(const ishara_model* m) { return (int32_t)m->entries.size(); }
extern "C" int ishara_param_info(const ishara_model* m, int32_t i, const char** name, int32_t* ndim, int64_t shape[2], int64_t* offset, int32_t* trainable) {
    if (i < 0 || i >= (int)m->entries.size()) { ishara_set_error("param index out of range"); return -1; }
    const ParamEntry& e = m->entries[i];
    if (name) *name = e.name.c_str();
    if (ndim) *ndim = e.ndim;
    if (shape) { shape[0] = e.shape[0]; shape[1] = e.shape[1]; }
    if (offset) *offset = e.offset;
    if (trainable) *trainable = e.trainable ? 1 : 0;
    return 0;
}
extern "C" int64_t ishara_workspace_bytes(const ishara_model* m) { return (int64_t)m->ws_need; }
// Host-side audit of the workspace plan: every buffer 256-byte aligned, inside [0, workspace_bytes), no two buffers (or guard
// zones) overlapping.  Returns the number of buffers, <0 on a violation.
extern "C" int32_t ishara_workspace_plan_check(const ishara_model* m) {
    std::vector<std::pair<size_t, size_t>> r = m->allocs;
    for (size_t off : m->guard_offs) r.push_back({off, 256});
    std::sort(r.begin(), r.end());
    size_t end = 0;
    for (auto& a : r) {
        if (a.first % 256 != 0) { ishara_set_error("workspace buffer at %zu is not 256-byte aligned", a.first); return -1; }
        if (a.first < end) { ishara_set_error("workspace buffers overlap at offset %zu (previous buffer ends at %zu)", a.first, end); return -1; }
        end = a.first + a.second;
        if (end > m->ws_need) { ishara_set_error("workspace buffer [%zu, %zu) exceeds the planned size %zu", a.first, end, m->ws_need); return -1; }
    }
    return (int32_t)m->allocs.size();
}
// Guard zones (ISHARA_WS_GUARD=1 at create): synchronises the device, returns 0 when every guard still holds its pattern, else -3
// with the workspace offset of the first damaged guard (and the buffer in front of it) in ishara_last_error().  0 guards: returns 0.
extern "C" int ishara_workspace_guard_check(ishara_model* m) {
    if (!m->guard || !m->ws) return 0;
    HIP_CHECK_RET(hipDeviceSynchronize());
    std::vector<uint32_t> got(64);
    for (size_t gi = 0; gi < m->guard_offs.size(); ++gi) {
        HIP_CHECK_RET(hipMemcpy(got.data(), m->ws + m->guard_offs[gi], 256, hipMemcpyDeviceToHost));
        for (int i = 0; i < 64; ++i)
            if (got[i] != 0xA5C3A5C3u) {
                size_t boff = 0, bsz = 0;
                for (auto& a : m->allocs) if (a.first < m->guard_offs[gi] && a.first >= boff) { boff = a.first; bsz = a.second; }
                ishara_set_error("workspace guard %zu at offset %zu damaged at byte %d (value 0x%08x): the buffer in front of it is [%zu, %zu)",
                                 gi, m->guard_offs[gi], i * 4, got[i], boff, boff + bsz);
                return -3;
            }
    }
    return 0;
}

extern "C" int ishara_bind(ishara_model* m, float* params, float* grads, float* opt_m, float* opt_v, float* opt_slow, void* workspace, int64_t workspace_bytes) {
    if (!params || !workspace) { ishara_set_error("ishara_bind: params and workspace are required"); return -1; }
    if ((size_t)workspace_bytes < m->ws_need) { ishara_set_error("ishara_bind: workspace too small (%lld < %zu)", (long long)workspace_bytes, m->ws_need); return -1; }
    if (((uintptr_t)workspace) % 256 != 0) { ishara_set_error("ishara_bind: workspace must be 256-byte aligned"); return -1; }
    m->params = params; m->grads = grads; m->om = opt_m; m->ov = opt_v; m->oslow = opt_slow;
    m->ws = (char*)workspace; m->ws_bytes = workspace_bytes;
    m->shadow_ready = false;               // new buffers: rebuild the descriptor table and re-zero the padding
    if (m->guard) {
        std::vector<uint32_t> pat(64, 0xA5C3A5C3u);
        for (size_t off : m->guard_offs) HIP_CHECK_RET(hipMemcpy(m->ws + off, pat.data(), 256, hipMemcpyHostToDevice));
    }
    if (m->family == ISHARA_FAMILY_TORCH_SQUEEZEFORMER) CK(r4_bind(m));
    if (m->family == ISHARA_FAMILY_KERAS_HYBRID) HIP_CHECK_RET(hipMemcpy(m->ws + m->pe.off, m->pe_host.data(), m->pe_host.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int ishara_sync_weights(ishara_model* m, ishara_stream st) {
    hipStream_t s = (hipStream_t)st;
    if (!m->ws) { ishara_set_error("not bound"); return -1; }
    // the zero padding of the shadow arena is written once; afterwards every step rewrites only the [K, N] interiors, all
    // weights in one launch (63 launches + a fill of the arena were 0.23 ms of a 21 ms step)
    if (!m->shadow_ready) {
        HIP_CHECK_RET(hipMemsetAsync(m->ws + m->shadow_begin, 0, m->shadow_end - m->shadow_begin, s));
        if (m->guard) {                          // the arena fill above also cleared the guard zones between the shadows: re-arm them
            static const std::vector<uint32_t> pat(64, 0xA5C3A5C3u);
            for (size_t off : m->guard_offs)
                if (off >= m->shadow_begin && off < m->shadow_end) HIP_CHECK_RET(hipMemcpyAsync(m->ws + off, pat.data(), 256, hipMemcpyHostToDevice, s));
        }
        std::vector<ShadowDesc> tab;
        int tile0 = 0;
        for (DenseW* w : m->denses) {
            ShadowDesc d;
            d.W = m->P(w->w); d.Wt = m->ws + w->wt; d.Wn = m->ws + w->wn; d.K = w->K; d.N = w->N; d.ldt = w->ldt; d.ldn = w->ldn;
            d.tile0 = tile0; d.tiles_n = (w->N + 31) / 32;
            tile0 += d.tiles_n * ((w->K + 31) / 32);
            tab.push_back(d);
        }
        m->shadow_tiles = tile0;
        m->shadow_ntab = (int)tab.size();
        m->shadow_tab_host = tab;
        HIP_CHECK_RET(hipMemcpyAsync(m->ws + m->shadow_tab_off, m->shadow_tab_host.data(), tab.size() * sizeof(ShadowDesc), hipMemcpyHostToDevice, s));
        m->shadow_ready = true;
    }
    CK(launch_make_shadow_batched(m->dt, reinterpret_cast<const ShadowDesc*>(m->ws + m->shadow_tab_off), m->shadow_ntab, m->shadow_tiles, s));
    return 0;
}

// ------------------------------------------------------------------ GEMM wrappers
int gemm_fwd(ishara_model* m, const DenseW& w, const void* A, int dtA, void* Cc, int dtC, int M, int aop, const OpArgs& oa, EpiArgs ea) {
    if (w.b >= 0) ea.bias = m->P(w.b);
    const double by = (double)M * w.K * dt_size(dtA) + (double)M * w.N * dt_size(dtC) * (1 + (ea.resid ? 1 : 0) + (ea.pre_out ? 1 : 0)) + (double)w.K * w.N * dt_size(m->dt);
    CKP(m, gemm_nt_kernel_name(dtA, m->dt, dtC, aop, A, M, w.N, w.K, w.ldt, ea), by, 2.0 * M * w.N * w.K, launch_gemm_nt(dtA, m->dt, dtC, aop, A, m->ws + w.wt, Cc, M, w.N, w.K, w.ldt, oa, ea, m->s));
    return 0;
}
int gemm_dgrad(ishara_model* m, const DenseW& w, const void* dY, int dtA, void* dX, int M, int aop, const OpArgs& oa, const EpiArgs& ea) {
    const double by = (double)M * w.N * dt_size(dtA) + (double)M * w.K * dt_size(m->dt) * (1 + (ea.resid ? 1 : 0) + (ea.aux ? 1 : 0)) + (double)w.K * w.N * dt_size(m->dt);
    CKP(m, gemm_nt_kernel_name(dtA, m->dt, m->dt, aop, dY, M, w.K, w.N, w.ldn, ea), by, 2.0 * M * w.N * w.K, launch_gemm_nt(dtA, m->dt, m->dt, aop, dY, m->ws + w.wn, dX, M, w.K, w.N, w.ldn, oa, ea, m->s));
    return 0;
}
// ---- deferred parameter-gradient sums (kernels.h RedSink): the LayerNorm / depthwise-conv backward operators leave their partial rows in a
// bump arena instead of the shared slab, and ONE launch at the end of the backward pass (or when the arena / job table is full, or before a
// gradient bucket is declared final) sums them all.  Off: ISHARA_NO_DEFERRED_REDUCE=1.
int red_flush(ishara_model* m) {
    if (m->red.njobs == 0) { m->red_off = 0; return 0; }
    CKP(m, "reduce_jobs(deferred)", 0, 0, launch_reduce_flush(&m->red, m->s));
    m->red_off = 0;
    return 0;
}
static float* red_scratch(ishara_model* m, size_t floats) {
    if (!m->red_on || floats > m->red_cap) return m->Wf(m->slab);
    floats = (floats + 63) & ~(size_t)63;
    if (m->red_off + floats > m->red_cap || reduce_sink_full()) { g_red_sink = nullptr; (void)red_flush(m); }
    g_red_sink = &m->red;
    float* p = m->Wf(m->red_arena) + m->red_off;
    m->red_off += floats;
    return p;
}
struct RedScope {      // the sink is installed by red_scratch (only for operators that got arena scratch) and removed when the launch returns
    ~RedScope() { g_red_sink = nullptr; }
};
// dx = LayerNorm backward of dy at x (+ resid), dgamma / dbeta accumulated through the deferred sums
int layernorm_bwd_deferred(ishara_model* m, const Run& r, const void* dy, const void* x, Buf mean, Buf rstd, const Norm& ln, const void* resid, void* dx) {
    RedScope scope;
    CKP(m, "layernorm_bwd", 4.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_layernorm_bwd(m->dt, dy, x, m->Wf(mean), m->Wf(rstd), m->P(ln.gamma), resid, dx, m->G(ln.gamma), m->G(ln.beta), red_scratch(m, layernorm_bwd_scratch_floats(m->d)), r.M, m->d, m->s));
    return 0;
}
// depthwise-conv backward over C channels (parameter entries dw, dwb; dwb < 0: no bias), the kernel gradient through the deferred sums.
// bn: the BatchNorm backward applied inside (one pass over dy, bn->h and x) where the fused kernel takes the shape.  Returns < 0 on an
// error, 1 when the fused kernel ran, else 0 (bn given: the caller takes the two-kernel path).  by_factor: passes over [M, d] the profiler books.
int dwconv_bwd_deferred(ishara_model* m, const Run& r, double by_factor, int inop, const void* dy, const DwBnArgs* bn, const void* x, int dw, int dwb, void* dx, int C, int k, int padl) {
    RedScope scope;
    float* dbias = dwb >= 0 ? m->G(dwb) : nullptr;
    int fused = 0;
    if (bn) CKP(m, "dwconv_bwd", by_factor * r.M * m->d * (double)dt_size(m->dt), 0, (fused = launch_dwconv_bwd_bn(m->dt, inop, dy, *bn, x, m->P(dw), dx, m->G(dw), dbias, red_scratch(m, dwconv_bwd_scratch_floats(C, k)), r.B, m->T, C, k, padl, m->s)) < 0 ? fused : 0);
    else CKP(m, "dwconv_bwd", by_factor * r.M * m->d * (double)dt_size(m->dt), 0, launch_dwconv_bwd(m->dt, inop, dy, x, m->P(dw), dx, m->G(dw), dbias, red_scratch(m, dwconv_bwd_scratch_floats(C, k)), r.B, m->T, C, k, padl, m->s));
    return fused;
}
// gradient through an output dropout (site, rate): g itself when the site drops nothing, else the masked and scaled rows in tmp
const void* grad_through_dropout(ishara_model* m, const Run& r, uint32_t site, float rate, const void* g, void* tmp, int T, int cols, int* rc) {
    const DropSpec od = dspec(r, site, rate);
    *rc = 0;
    if (!od.thr) return g;
    *rc = [&]() -> int {
        CKP(m, "map_rows", 2.0 * r.M * cols * (double)dt_size(m->dt), 0, launch_map_rows(m->dt, MAP_DROPMASK, g, tmp, nullptr, od, r.M, T, cols, m->s));
        return 0;
    }();
    return tmp;
}
int gemm_wgrad(ishara_model* m, const DenseW& w, const void* A, int dtA, int aop, const OpArgs& oa, const void* dY, int dtB, int bop, const OpArgs& ob, int M, int ka_valid, int nb_valid,
               const float* bias_rowscale, int bias_T, const TnPsa* psa) {
    const double by = (double)M * w.K * dt_size(dtA) + (double)M * w.N * dt_size(dtB) + (double)w.K * w.N * 4;
    // the GEMM kernel and the sums of its split-M slabs are profiled under separate keys (the kernel's key is its rocprof name)
    if (m->tn_defer_on && !m->prof.on) {       // the sums of this GEMM's slabs ride with the next weight-gradient GEMM (gemm_tn.hip, TnDefer)
        m->tn_defer.slab[0] = m->Wf(m->slab2[0]); m->tn_defer.slab[1] = m->Wf(m->slab2[1]);
        return launch_gemm_tn(dtA, dtB, m->dt, aop, bop, A, dY, m->G(w.w), w.b >= 0 ? m->G(w.b) : nullptr, m->Wf(m->slab), M, w.K, w.N, oa, ob, m->s, ka_valid, nb_valid, bias_rowscale, bias_T, &m->tn_defer, psa);
    }
    g_tn_phase = 1;
    CKP(m, gemm_tn_kernel_name(dtA, dtB, m->dt, aop, bop, M, w.K, w.N, ka_valid, nb_valid, bias_rowscale, bias_T, psa), by, 2.0 * M * w.N * w.K, launch_gemm_tn(dtA, dtB, m->dt, aop, bop, A, dY, m->G(w.w), w.b >= 0 ? m->G(w.b) : nullptr, m->Wf(m->slab), M, w.K, w.N, oa, ob, m->s, ka_valid, nb_valid, bias_rowscale, bias_T, nullptr, psa));
    g_tn_phase = 2;
    CKP(m, "reduce_slabs(wgrad)", 0, 0, launch_gemm_tn(dtA, dtB, m->dt, aop, bop, A, dY, m->G(w.w), w.b >= 0 ? m->G(w.b) : nullptr, m->Wf(m->slab), M, w.K, w.N, oa, ob, m->s, ka_valid, nb_valid, bias_rowscale, bias_T, nullptr, psa));
    g_tn_phase = 0;
    return 0;
}

int wgrad_flush(ishara_model* m) { return launch_gemm_tn_flush(&m->tn_defer, m->s); }

// ---- gradient buckets (overlapping the data-parallel all-reduce with the backward pass)
extern "C" int32_t ishara_grad_buckets(const ishara_model* m) { return (int32_t)m->bucket_lo.size(); }
extern "C" int ishara_grad_bucket(const ishara_model* m, int32_t i, int64_t* offset, int64_t* count) {
    if (i < 0 || i >= (int32_t)m->bucket_lo.size()) { ishara_set_error("ishara_grad_bucket: index %d outside 0..%d", i, (int)m->bucket_lo.size() - 1); return -1; }
    *offset = m->bucket_lo[i]; *count = m->bucket_hi[i] - m->bucket_lo[i];
    return 0;
}
// makes `side` wait until bucket i of the LAST ishara_loss_backward is final (events are created on first use)
extern "C" int ishara_grad_bucket_wait(ishara_model* m, int32_t i, ishara_stream side) {
    if (i < 0 || i >= (int32_t)m->bucket_lo.size()) { ishara_set_error("ishara_grad_bucket_wait: index %d outside 0..%d", i, (int)m->bucket_lo.size() - 1); return -1; }
    if (m->bucket_ev.empty()) { ishara_set_error("ishara_grad_bucket_wait: call ishara_grad_buckets_enable before the backward pass"); return -1; }
    HIP_CHECK_RET(hipStreamWaitEvent((hipStream_t)side, m->bucket_ev[i], 0));
    return 0;
}
extern "C" int ishara_grad_buckets_enable(ishara_model* m) {
    if (!m->bucket_ev.empty()) return 0;
    m->bucket_ev.resize(m->bucket_lo.size());
    for (auto& e : m->bucket_ev) HIP_CHECK_RET(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return 0;
}

// ------------------------------------------------------------------ optimizer
// groups != nullptr: the grouped update (parameter groups) in place of the plain one; everything around it is the same
static int optimizer_step(ishara_model* m, const char* who, float lr, float weight_decay, const float* grad, ishara_grad_stats* rec, int skip, ishara_stream st,
                          const int64_t* seg_off = nullptr, const ishara_param_group* groups = nullptr, int32_t S = 0, void* ws = nullptr) {
    if (!m->om || !m->ov || !m->oslow || !m->grads) { ishara_set_error("%s: optimizer slots are not bound", who); return -1; }
    hipStream_t s = (hipStream_t)st;
    m->opt_iter += 1;
    const RAdamArgs a = radam_args(m->opt_iter, lr, weight_decay);
    m->s = s;
    if (!grad) grad = m->grads;
    if (groups) CKP(m, "radam_lookahead_groups", 28.0 * m->n_train, 0, launch_radam_lookahead_groups(m->params, grad, m->om, m->ov, m->oslow, m->n_train, a, rec, skip, seg_off, groups, S, ws, s));
    else if (rec) CKP(m, "radam_lookahead", 28.0 * m->n_train, 0, launch_radam_lookahead_ex(m->params, grad, m->om, m->ov, m->oslow, m->n_train, a, rec, skip, s));
    else CKP(m, "radam_lookahead", 28.0 * m->n_train, 0, launch_radam_lookahead(m->params, grad, m->om, m->ov, m->oslow, m->n_train, a, s));
    CKP(m, "weight_shadows", 0, 0, ishara_sync_weights(m, st));      // also after a skipped step: the host cannot know it was one
    return 0;
}
extern "C" int ishara_optimizer_step(ishara_model* m, float lr, float weight_decay, ishara_stream st) {
    return optimizer_step(m, "ishara_optimizer_step", lr, weight_decay, nullptr, nullptr, 0, st);
}
extern "C" int ishara_optimizer_step_ex(ishara_model* m, float lr, float weight_decay, const float* grad, ishara_grad_stats* rec, int32_t skip_nonfinite,
                                        ishara_stream st) {
    const char* who = "ishara_optimizer_step_ex";
    if (!m) { ishara_set_error("%s: null handle", who); return -1; }
    if ((uintptr_t)grad % 16 != 0) { ishara_set_error("%s: misaligned grad: %p is not on a 16-byte boundary", who, (const void*)grad); return -1; }
    if ((uintptr_t)rec % 4 != 0) { ishara_set_error("%s: misaligned st: %p is not on a 4-byte boundary", who, (void*)rec); return -1; }
    if (skip_nonfinite && !rec) { ishara_set_error("%s: skip_nonfinite needs the record: null st", who); return -1; }
    return optimizer_step(m, who, lr, weight_decay, grad, rec, skip_nonfinite != 0, st);
}

// ------------------------------------------------------------------ gradient statistics / accumulation (grad_ops.hip)
static bool grad_vec_ok(const char* who, std::initializer_list<std::pair<const char*, const void*>> ps, int64_t n) {
    for (auto& p : ps) if (!p.second) { ishara_set_error("%s: null %s", who, p.first); return false; }
    for (auto& p : ps) if ((uintptr_t)p.second % 16 != 0) { ishara_set_error("%s: misaligned %s: %p is not on a 16-byte boundary", who, p.first, p.second); return false; }
    if (n < 1 || n > 2147483647LL) { ishara_set_error("%s: n=%lld is outside 1..2147483647", who, (long long)n); return false; }
    return true;
}
extern "C" int64_t ishara_grad_stats_workspace_bytes(int64_t n) {
    if (n < 1 || n > 2147483647LL) { ishara_set_error("ishara_grad_stats_workspace_bytes: n=%lld is outside 1..2147483647", (long long)n); return -1; }
    return grad_stats_workspace_bytes(n);
}
extern "C" int ishara_gradient_stats(ishara_model* prof, const float* g, int64_t n, float grad_scale, float clip_norm, ishara_grad_stats* out, void* ws,
                                     ishara_stream st) {
    const char* who = "ishara_gradient_stats";
    if (!grad_vec_ok(who, {{"g", g}}, n)) return -1;
    if (!out || !ws) { ishara_set_error("%s: null %s", who, !out ? "out" : "ws"); return -1; }
    if ((uintptr_t)out % 4 != 0) { ishara_set_error("%s: misaligned out: %p is not on a 4-byte boundary", who, (void*)out); return -1; }
    if ((uintptr_t)ws % 8 != 0) { ishara_set_error("%s: misaligned ws: %p is not on an 8-byte boundary", who, ws); return -1; }
    if (!(grad_scale >= 0.f) || std::isinf(grad_scale)) { ishara_set_error("%s: grad_scale %g is not a finite value >= 0", who, (double)grad_scale); return -1; }
    if (std::isnan(clip_norm)) { ishara_set_error("%s: clip_norm is NaN", who); return -1; }
    hipStream_t s = (hipStream_t)st;
    if (!prof) return launch_grad_stats(g, n, grad_scale, clip_norm, out, ws, s);
    prof->s = s;
    CKP(prof, "grad_stats", 4.0 * n, 0, launch_grad_stats(g, n, grad_scale, clip_norm, out, ws, s));
    return 0;
}
extern "C" int ishara_gradient_accumulate(ishara_model* prof, float* acc, const float* g, int64_t n, int32_t first, ishara_stream st) {
    const char* who = "ishara_gradient_accumulate";
    if (!grad_vec_ok(who, {{"acc", acc}, {"g", g}}, n)) return -1;
    if (acc == g) { ishara_set_error("%s: acc and g are the same buffer", who); return -1; }
    hipStream_t s = (hipStream_t)st;
    if (!prof) return launch_grad_accumulate(acc, g, n, first != 0, s);
    prof->s = s;
    CKP(prof, "grad_accumulate", 12.0 * n, 0, launch_grad_accumulate(acc, g, n, first != 0, s));
    return 0;
}
// ------------------------------------------------------------------ exponential moving average of the weights (weight_avg.hip)
static bool ranges_overlap(const float* a, const float* b, int64_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b, bytes = (uintptr_t)n * sizeof(float);
    return x < y + bytes && y < x + bytes;
}
extern "C" int ishara_weight_average(ishara_model* prof, float* avg, float* theta, int64_t n, float momentum, int32_t warmup, int32_t overwrite_every,
                                     ishara_ema_state* rec, const ishara_grad_stats* stats, int32_t skip_nonfinite, ishara_stream st) {
    const char* who = "ishara_weight_average";
    if (!grad_vec_ok(who, {{"avg", avg}, {"theta", theta}}, n)) return -1;
    if (!rec) { ishara_set_error("%s: null rec", who); return -1; }
    if ((uintptr_t)rec % 8 != 0) { ishara_set_error("%s: misaligned rec: %p is not on an 8-byte boundary", who, (void*)rec); return -1; }
    if (ranges_overlap(avg, theta, n)) { ishara_set_error("%s: avg and theta overlap", who); return -1; }
    if (!(momentum >= 0.f && momentum < 1.f)) { ishara_set_error("%s: momentum %g is outside [0, 1)", who, (double)momentum); return -1; }
    if (overwrite_every < 0) { ishara_set_error("%s: overwrite_every=%d is negative", who, (int)overwrite_every); return -1; }
    if (skip_nonfinite && !stats) { ishara_set_error("%s: skip_nonfinite needs the record: null st", who); return -1; }
    if ((uintptr_t)stats % 4 != 0) { ishara_set_error("%s: misaligned st: %p is not on a 4-byte boundary", who, (const void*)stats); return -1; }
    hipStream_t s = (hipStream_t)st;
    if (!prof) return launch_weight_average(avg, theta, n, momentum, warmup != 0, overwrite_every, rec, stats, skip_nonfinite != 0, s);
    prof->s = s;
    CKP(prof, "weight_average", (overwrite_every > 0 ? 16.0 : 12.0) * n, 0,
        launch_weight_average(avg, theta, n, momentum, warmup != 0, overwrite_every, rec, stats, skip_nonfinite != 0, s));
    return 0;
}
extern "C" int ishara_weight_swap(ishara_model* prof, float* a, float* b, int64_t n, ishara_stream st) {
    const char* who = "ishara_weight_swap";
    if (!grad_vec_ok(who, {{"a", a}, {"b", b}}, n)) return -1;
    if (ranges_overlap(a, b, n)) { ishara_set_error("%s: a and b overlap", who); return -1; }
    hipStream_t s = (hipStream_t)st;
    if (!prof) return launch_weight_swap(a, b, n, s);
    prof->s = s;
    CKP(prof, "weight_swap", 16.0 * n, 0, launch_weight_swap(a, b, n, s));
    return 0;
}
// ------------------------------------------------------------------ adversarial weight perturbation (awp.hip)
static bool awp_count_ok(const char* who, int64_t n) {
    if (n < 1 || n > 2147483647LL) { ishara_set_error("%s: n=%lld is outside 1..2147483647", who, (long long)n); return false; }
    return true;
}
static bool awp_ptr_ok(const char* who, const char* name, const void* p, int align) {
    if (!p) { ishara_set_error("%s: null %s", who, name); return false; }
    if ((uintptr_t)p % align != 0) { ishara_set_error("%s: misaligned %s: %p is not on a %d-byte boundary", who, name, p, align); return false; }
    return true;
}
extern "C" int64_t ishara_awp_workspace_bytes(int64_t n, int32_t S) {
    const char* who = "ishara_awp_workspace_bytes";
    if (!awp_count_ok(who, n)) return -1;
    if (S < 1 || S > n) { ishara_set_error("%s: S=%d is outside 1..n=%lld", who, (int)S, (long long)n); return -1; }
    return awp_workspace_bytes(n, S);
}
extern "C" int ishara_awp_perturb(ishara_model* prof, float* w, float* backup, const float* g, const int64_t* seg_off, int32_t S, int64_t n,
                                  float delta, float eps, int32_t relative, float* scale, ishara_awp_stats* rec, void* ws, ishara_stream st) {
    const char* who = "ishara_awp_perturb";
    if (!awp_ptr_ok(who, "w", w, 16) || !awp_ptr_ok(who, "backup", backup, 16) || !awp_ptr_ok(who, "g", g, 4) || !awp_ptr_ok(who, "seg_off", seg_off, 8) ||
        !awp_ptr_ok(who, "scale", scale, 4) || !awp_ptr_ok(who, "rec", rec, 4) || !awp_ptr_ok(who, "ws", ws, 8)) return -1;
    if (!awp_count_ok(who, n)) return -1;
    if (S < 1 || S > n) { ishara_set_error("%s: S=%d is outside 1..n=%lld", who, (int)S, (long long)n); return -1; }
    if (ranges_overlap(w, backup, n)) { ishara_set_error("%s: w and backup overlap", who); return -1; }
    if (!(delta > 0.f) || std::isinf(delta)) { ishara_set_error("%s: delta %g is not a finite value > 0", who, (double)delta); return -1; }
    if (!(eps > 0.f) || std::isinf(eps)) { ishara_set_error("%s: eps %g is not a finite value > 0", who, (double)eps); return -1; }
    hipStream_t s = (hipStream_t)st;
    if (!prof) {
        CK(launch_awp_norms(w, g, seg_off, S, n, delta, eps, relative != 0, scale, rec, ws, s));
        return launch_awp_apply(w, backup, g, seg_off, S, n, scale, ws, s);
    }
    prof->s = s;
    CKP(prof, "awp_norms", (relative ? 8.0 : 4.0) * n, 0, launch_awp_norms(w, g, seg_off, S, n, delta, eps, relative != 0, scale, rec, ws, s));
    CKP(prof, "awp_perturb", 16.0 * n, 0, launch_awp_apply(w, backup, g, seg_off, S, n, scale, ws, s));
    return 0;
}
extern "C" int ishara_awp_restore(ishara_model* prof, float* w, const float* backup, int64_t n, ishara_stream st) {
    const char* who = "ishara_awp_restore";
    if (!awp_ptr_ok(who, "w", w, 16) || !awp_ptr_ok(who, "backup", backup, 16)) return -1;
    if (!awp_count_ok(who, n)) return -1;
    if (ranges_overlap(w, backup, n)) { ishara_set_error("%s: w and backup overlap", who); return -1; }
    hipStream_t s = (hipStream_t)st;
    if (!prof) return launch_awp_restore(w, backup, n, s);
    prof->s = s;
    CKP(prof, "awp_restore", 8.0 * n, 0, launch_awp_restore(w, backup, n, s));
    return 0;
}
// ------------------------------------------------------------------ optimizer parameter groups (optimizer.hip)
static bool groups_table_ok(const char* who, const int64_t* seg_off, const ishara_param_group* groups, int32_t S, int64_t n, const void* ws) {
    if (!awp_ptr_ok(who, "seg_off", seg_off, 8) || !awp_ptr_ok(who, "groups", groups, 4) || !awp_ptr_ok(who, "ws", ws, 8)) return false;
    if (S < 1 || S > n) { ishara_set_error("%s: S=%d is outside 1..n=%lld", who, (int)S, (long long)n); return false; }
    return true;
}
static bool step_record_ok(const char* who, const ishara_grad_stats* rec, int32_t skip_nonfinite) {
    if ((uintptr_t)rec % 4 != 0) { ishara_set_error("%s: misaligned st: %p is not on a 4-byte boundary", who, (const void*)rec); return false; }
    if (skip_nonfinite && !rec) { ishara_set_error("%s: skip_nonfinite needs the record: null st", who); return false; }
    return true;
}
static bool op_step_ok(const char* who, float* theta, const float* grad, float* m, float* v, float* slow, int64_t n, int32_t iteration,
                       const ishara_grad_stats* rec, int32_t skip_nonfinite) {
    if (!awp_ptr_ok(who, "theta", theta, 16) || !awp_ptr_ok(who, "grad", grad, 16) || !awp_ptr_ok(who, "m", m, 16) || !awp_ptr_ok(who, "v", v, 16) ||
        !awp_ptr_ok(who, "slow", slow, 16)) return false;
    if (!awp_count_ok(who, n)) return false;
    if (iteration < 1) { ishara_set_error("%s: iteration=%d is not >= 1", who, (int)iteration); return false; }
    return step_record_ok(who, rec, skip_nonfinite);
}
extern "C" int64_t ishara_param_groups_workspace_bytes(int64_t n, int32_t S) {
    const char* who = "ishara_param_groups_workspace_bytes";
    if (!awp_count_ok(who, n)) return -1;
    if (S < 1 || S > n) { ishara_set_error("%s: S=%d is outside 1..n=%lld", who, (int)S, (long long)n); return -1; }
    return param_groups_workspace_bytes(n, S);
}
extern "C" int ishara_optimizer_step_groups(ishara_model* m, float lr, float weight_decay, const float* grad, ishara_grad_stats* rec, int32_t skip_nonfinite,
                                            const int64_t* seg_off, const ishara_param_group* groups, int32_t S, void* ws, ishara_stream st) {
    const char* who = "ishara_optimizer_step_groups";
    if (!m) { ishara_set_error("%s: null handle", who); return -1; }
    if ((uintptr_t)grad % 16 != 0) { ishara_set_error("%s: misaligned grad: %p is not on a 16-byte boundary", who, (const void*)grad); return -1; }
    if (!step_record_ok(who, rec, skip_nonfinite)) return -1;
    if (!awp_ptr_ok(who, "seg_off", seg_off, 8) || !awp_ptr_ok(who, "groups", groups, 4) || !awp_ptr_ok(who, "ws", ws, 8)) return -1;      // before the handle is read
    if (!awp_count_ok(who, m->n_train) || !groups_table_ok(who, seg_off, groups, S, m->n_train, ws)) return -1;
    return optimizer_step(m, who, lr, weight_decay, grad, rec, skip_nonfinite != 0, st, seg_off, groups, S, ws);
}
extern "C" int ishara_gradient_mask_groups(ishara_model* prof, float* g, int64_t n, const int64_t* seg_off, const ishara_param_group* groups, int32_t S,
                                           void* ws, ishara_stream st) {
    const char* who = "ishara_gradient_mask_groups";
    if (!awp_ptr_ok(who, "g", g, 16)) return -1;
    if (!awp_count_ok(who, n) || !groups_table_ok(who, seg_off, groups, S, n, ws)) return -1;
    hipStream_t s = (hipStream_t)st;
    if (!prof) return launch_grad_mask_groups(g, n, seg_off, groups, S, ws, s);
    prof->s = s;
    CKP(prof, "grad_mask_groups", 4.0 * n, 0, launch_grad_mask_groups(g, n, seg_off, groups, S, ws, s));
    return 0;
}
extern "C" int ishara_optimizer_op_step(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n, int32_t iteration,
                                        float lr, float weight_decay, ishara_grad_stats* rec, int32_t skip_nonfinite, ishara_stream st) {
    const char* who = "ishara_optimizer_op_step";
    if (!op_step_ok(who, theta, grad, m, v, slow, n, iteration, rec, skip_nonfinite)) return -1;
    const RAdamArgs a = radam_args(iteration, lr, weight_decay);
    if (rec) return launch_radam_lookahead_ex(theta, grad, m, v, slow, n, a, rec, skip_nonfinite != 0, (hipStream_t)st);
    return launch_radam_lookahead(theta, grad, m, v, slow, n, a, (hipStream_t)st);
}
extern "C" int ishara_optimizer_op_step_groups(float* theta, const float* grad, float* m, float* v, float* slow, int64_t n, int32_t iteration,
                                               float lr, float weight_decay, ishara_grad_stats* rec, int32_t skip_nonfinite,
                                               const int64_t* seg_off, const ishara_param_group* groups, int32_t S, void* ws, ishara_stream st) {
    const char* who = "ishara_optimizer_op_step_groups";
    if (!op_step_ok(who, theta, grad, m, v, slow, n, iteration, rec, skip_nonfinite) || !groups_table_ok(who, seg_off, groups, S, n, ws)) return -1;
    return launch_radam_lookahead_groups(theta, grad, m, v, slow, n, radam_args(iteration, lr, weight_decay), rec, skip_nonfinite != 0, seg_off, groups, S, ws,
                                         (hipStream_t)st);
}
extern "C" int32_t ishara_optimizer_iterations(const ishara_model* m) { return m->opt_iter; }
extern "C" int ishara_optimizer_set_iterations(ishara_model* m, int32_t it) { m->opt_iter = it; return 0; }

// ------------------------------------------------------------------ profiler API
extern "C" int ishara_profile_enable(ishara_model* m, int32_t on) {
    m->prof.on = on != 0;
    m->prof.recs.clear();
    m->prof.used = 0;
    return 0;
}
// one text line per kernel family: "key count total_ms bytes flops\n"; returns bytes written (or <0)
extern "C" int ishara_profile_report(ishara_model* m, char* buf, int32_t cap) {
    struct Agg { int n = 0; double ms = 0, by = 0, fl = 0; };
    std::map<std::string, Agg> agg;
    std::vector<std::string> order;
    for (auto& r : m->prof.recs) {
        if (hipEventSynchronize(r.e1) != hipSuccess) { ishara_set_error("profile: event sync failed"); return -2; }
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, r.e0, r.e1);
        if (!agg.count(r.key)) order.push_back(r.key);
        Agg& a = agg[r.key];
        a.n++; a.ms += ms; a.by += r.bytes; a.fl += r.flops;
    }
    int pos = 0;
    for (auto& k : order) {
        const Agg& a = agg[k];
        const int w = snprintf(buf + pos, cap > pos ? cap - pos : 0, "%s %d %.6f %.0f %.0f\n", k.c_str(), a.n, a.ms, a.by, a.fl);
        if (w < 0 || pos + w >= cap) { ishara_set_error("profile: buffer too small"); return -1; }
        pos += w;
    }
    m->prof.recs.clear();
    m->prof.used = 0;
    return pos;
}
