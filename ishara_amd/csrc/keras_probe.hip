// The module probe of the Keras get_model hybrid (debug aid; tests/test_modules_gpu.py): ishara_debug_module_* and
// ishara_debug_head_loss_backward run one module of the sequential graph alone through the module functions of conv_block.hip and
// keras_hybrid.hip.
#include "model_types.h"

// ------------------------------------------------------------------ module probe (debug aid; tests/test_modules_gpu.py)
// One module of the sequential graph run alone through the functions above, with the model's own Run, site ids and switches: its input
// sits where the model has it (the output buffer of the module in front), gradients travel through gA / gB.  No buffer of its own.
struct ProbeMod {
    enum Kind { STEM, CONV, FFN_, MHSA_, SQZCONV, CONFCONV, HEAD } kind;
    std::string name; int in_cols, out_cols; uint32_t first_site, n_sites;
    void* ptr;            // ConvBlock / FFN / MHSA / SqzConv / ConfConv
    Buf in, out;          // module input / output activation (STEM: no input buffer; HEAD: no output buffer)
};
static std::vector<ProbeMod> probe_modules(ishara_model* m) {
    std::vector<ProbeMod> v;
    uint32_t site = 0;
    Buf prev = m->stem_out;
    auto add = [&](ProbeMod::Kind k, const std::string& name, int in_cols, int out_cols, uint32_t n_sites, void* ptr, Buf out) {
        v.push_back(ProbeMod{k, name, in_cols, out_cols, site, n_sites, ptr, prev, out});
        site += n_sites; prev = out;
    };
    const int d = m->d;
    add(ProbeMod::STEM, "stem", m->F, d, 0, nullptr, m->stem_out);
    for (const Layer& L : m->layers) {
        if (L.kind == Layer::CONV) {
            ConvBlock& cb = m->convs[L.idx];
            const std::string& n = m->entries[cb.W1.w].name;                 // "<prefix>_expand_conv/kernel"
            add(ProbeMod::CONV, n.substr(0, n.size() - strlen("_expand_conv/kernel")), d, d, 1, &cb, cb.out);
        } else if (L.kind == Layer::SQZ) {
            SqzBlock& sb = m->sqz[L.idx];
            const std::string n = "squeezeformer_" + std::to_string(L.idx);
            add(ProbeMod::FFN_, n + "/ffn1", d, d, 1 + (sb.ffn1.has_out_drop ? 1 : 0), &sb.ffn1, sb.ffn1.out);
            add(ProbeMod::MHSA_, n + "/mha", d, d, 1 + (sb.mha.has_out_drop ? 1 : 0), &sb.mha, sb.mha.out);
            add(ProbeMod::SQZCONV, n + "/conv", d, d, 0, &sb.conv, sb.conv.out);
            add(ProbeMod::FFN_, n + "/ffn2", d, d, 1 + (sb.ffn2.has_out_drop ? 1 : 0), &sb.ffn2, sb.ffn2.out);
        } else {
            ConfBlock& cb = m->conf[L.idx];
            const std::string n = "conformer_" + std::to_string(L.idx);
            add(ProbeMod::FFN_, n + "/ffn1", d, d, 1 + (cb.ffn1.has_out_drop ? 1 : 0), &cb.ffn1, cb.ffn1.out);
            add(ProbeMod::MHSA_, n + "/mha", d, d, 1 + (cb.mha.has_out_drop ? 1 : 0), &cb.mha, cb.mha.out);
            add(ProbeMod::CONFCONV, n + "/conv", d, d, cb.conv.has_out_drop ? 1 : 0, &cb.conv, cb.conv.out);
            add(ProbeMod::FFN_, n + "/ffn2", d, d, 1 + (cb.ffn2.has_out_drop ? 1 : 0), &cb.ffn2, cb.ffn2.out);
        }
    }
    add(ProbeMod::HEAD, "head", d, m->C, 1, nullptr, Buf{});
    return v;
}
static bool probe_family_ok(const ishara_model* m, const char* fn) {
    if (!m) { ishara_set_error("%s: null handle", fn); return false; }
    if (m->family != ISHARA_FAMILY_KERAS_HYBRID) { ishara_set_error("%s: the module probe exists for ISHARA_FAMILY_KERAS_HYBRID only (family %d)", fn, m->family); return false; }
    return true;
}
extern "C" int32_t ishara_debug_module_count(ishara_model* m) {
    if (!probe_family_ok(m, "ishara_debug_module_count")) return -1;
    return (int32_t)probe_modules(m).size();
}
extern "C" int ishara_debug_module_info(ishara_model* m, int32_t i, const char** name, int32_t* in_cols, int32_t* out_cols, int32_t* first_site, int32_t* n_sites) {
    if (!probe_family_ok(m, "ishara_debug_module_info")) return -1;
    const std::vector<ProbeMod> v = probe_modules(m);
    if (i < 0 || i >= (int)v.size()) { ishara_set_error("ishara_debug_module_info: module index %d outside 0..%d", i, (int)v.size() - 1); return -1; }
    static thread_local std::string name_buf;      // valid until this thread's next call
    name_buf = v[i].name;
    if (name) *name = name_buf.c_str();
    if (in_cols) *in_cols = v[i].in_cols;
    if (out_cols) *out_cols = v[i].out_cols;
    if (first_site) *first_site = (int32_t)v[i].first_site;
    if (n_sites) *n_sites = (int32_t)v[i].n_sites;
    return 0;
}
// shared refusals of the probe's launching entry points: nothing is launched for a refused call
static bool probe_ok(ishara_model* m, const char* fn, int i, int B, const std::vector<ProbeMod>& v, int training, bool need_grads) {
    if (i < 0 || i >= (int)v.size()) { ishara_set_error("%s: module index %d outside 0..%d", fn, i, (int)v.size() - 1); return false; }
    if (B <= 0 || B > m->Bmax) { ishara_set_error("%s: batch %d outside 1..%d", fn, B, m->Bmax); return false; }
    if (m->dt == DT_F16 && training) { ishara_set_error("%s: ISHARA_F16 is an inference-only storage type: training=1 refused", fn); return false; }
    if (!m->ws || (need_grads && !m->grads)) { ishara_set_error("%s: model is not bound%s", fn, need_grads ? " (grads required)" : ""); return false; }
    return true;
}
static int probe_module_forward(const char* fn, ishara_model* m, int32_t i, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, const int32_t* frame_len, ishara_stream st) {
    if (!probe_family_ok(m, fn)) return -1;
    const std::vector<ProbeMod> v = probe_modules(m);
    if (!frame_len_ok(m, fn, frame_len)) return -1;
    if (!probe_ok(m, fn, i, B, v, training, false)) return -1;
    if (!x || !y) { ishara_set_error("%s: null x / y", fn); return -1; }
    m->s = (hipStream_t)st;
    m->probe_mod = -1; m->last_training = 0;      // the workspace no longer holds a whole forward pass: ishara_loss_backward refuses until the next ishara_forward
    const ProbeMod& p = v[i];
    Run r{B, B * m->T, training, seed};
    r.key_len = frame_len;
    const void* in = nullptr;
    if (p.kind != ProbeMod::STEM) { CK(r5_from_f32(m->dt, x, m->W(p.in), (size_t)r.M * p.in_cols, m->s)); in = m->W(p.in); }
    switch (p.kind) {
    case ProbeMod::STEM: CK(stem_fwd(m, r, x)); m->last_x = x; break;
    case ProbeMod::CONV: CK(conv_fwd(m, *(ConvBlock*)p.ptr, r, in)); break;
    case ProbeMod::FFN_: CK(ffn_fwd(m, *(FFN*)p.ptr, r, in)); break;
    case ProbeMod::MHSA_: CK(mhsa_fwd(m, *(MHSA*)p.ptr, r, in)); break;
    case ProbeMod::SQZCONV: CK(sqzconv_fwd(m, *(SqzConv*)p.ptr, r, in)); break;
    case ProbeMod::CONFCONV: CK(confconv_fwd(m, *(ConfConv*)p.ptr, r, in)); break;
    case ProbeMod::HEAD: CK(head_fwd(m, r, in, y)); break;
    }
    if (p.kind != ProbeMod::HEAD) CK(r5_to_f32(m->dt, m->W(p.out), y, (size_t)r.M * p.out_cols, m->s));
    if (training) { m->probe_mod = i; m->probe_B = B; m->probe_seed = seed; m->probe_masked = frame_len ? 1 : 0; }
    return 0;
}
extern "C" int ishara_debug_module_forward(ishara_model* m, int32_t i, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, ishara_stream st) {
    return probe_module_forward("ishara_debug_module_forward", m, i, x, B, y, training, seed, nullptr, st);
}
extern "C" int ishara_debug_module_forward_ex(ishara_model* m, int32_t i, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, const int32_t* frame_len, ishara_stream st) {
    return probe_module_forward("ishara_debug_module_forward_ex", m, i, x, B, y, training, seed, frame_len, st);
}
// zero gradients and empty deferred sums, as at the top of ishara_loss_backward
static int probe_backward_begin(ishara_model* m) {
    m->red.njobs = 0; m->red.nblocks = 0; m->red_off = 0; g_red_sink = nullptr;
    m->tn_defer.pending = false;
    return launch_fill_u32(m->grads, (size_t)m->n_train, 0u, m->s);
}
static int probe_module_backward(const char* fn, ishara_model* m, int32_t i, const float* dy, int32_t B, float* dx, const int32_t* frame_len, ishara_stream st) {
    if (!probe_family_ok(m, fn)) return -1;
    const std::vector<ProbeMod> v = probe_modules(m);
    if (!probe_ok(m, fn, i, B, v, 1, true)) return -1;
    if (m->probe_mod != i || m->probe_B != B) { ishara_set_error("%s: call ishara_debug_module_forward(training=1) of module %d with batch %d first", fn, i, B); return -1; }
    const ProbeMod& p = v[i];
    if (p.kind == ProbeMod::HEAD) { ishara_set_error("%s: the head's backward starts at the CTC kernel: use ishara_debug_head_loss_backward", fn); return -1; }
    if (!dy) { ishara_set_error("%s: null dy", fn); return -1; }
    if (p.kind == ProbeMod::STEM && dx) { ishara_set_error("%s: the stem has no input gradient: dx must be NULL", fn); return -1; }
    if (!frame_len_ok(m, fn, frame_len) || !frame_len_agrees(fn, m->probe_masked != 0, frame_len)) return -1;
    m->s = (hipStream_t)st;
    Run r{B, B * m->T, 1, m->probe_seed};
    r.key_len = frame_len;
    CK(probe_backward_begin(m));
    void* g = m->W(m->gA); void* gn = m->W(m->gB);
    CK(r5_from_f32(m->dt, dy, g, (size_t)r.M * p.out_cols, m->s));
    const void* in = p.kind == ProbeMod::STEM ? nullptr : m->W(p.in);
    switch (p.kind) {
    case ProbeMod::STEM: CK(stem_bwd(m, r, g)); break;
    case ProbeMod::CONV: CK(conv_bwd(m, *(ConvBlock*)p.ptr, r, in, g, gn)); break;
    case ProbeMod::FFN_: CK(ffn_bwd(m, *(FFN*)p.ptr, r, in, g, gn)); break;
    case ProbeMod::MHSA_: CK(mhsa_bwd(m, *(MHSA*)p.ptr, r, in, g, gn)); break;
    case ProbeMod::SQZCONV: CK(sqzconv_bwd(m, *(SqzConv*)p.ptr, r, in, g, gn)); break;
    case ProbeMod::CONFCONV: CK(confconv_bwd(m, *(ConfConv*)p.ptr, r, in, g, gn)); break;
    case ProbeMod::HEAD: break;
    }
    CK(wgrad_flush(m));
    CK(red_flush(m));
    if (dx) CK(r5_to_f32(m->dt, gn, dx, (size_t)r.M * p.in_cols, m->s));
    return 0;
}
extern "C" int ishara_debug_module_backward(ishara_model* m, int32_t i, const float* dy, int32_t B, float* dx, ishara_stream st) {
    return probe_module_backward("ishara_debug_module_backward", m, i, dy, B, dx, nullptr, st);
}
extern "C" int ishara_debug_module_backward_ex(ishara_model* m, int32_t i, const float* dy, int32_t B, float* dx, const int32_t* frame_len, ishara_stream st) {
    return probe_module_backward("ishara_debug_module_backward_ex", m, i, dy, B, dx, frame_len, st);
}
extern "C" int ishara_debug_head_loss_backward(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale, float* dx, ishara_stream st) {
    const char* fn = "ishara_debug_head_loss_backward";
    if (!probe_family_ok(m, fn)) return -1;
    const std::vector<ProbeMod> v = probe_modules(m);
    const int i = (int)v.size() - 1;
    if (!probe_ok(m, fn, i, B, v, 1, true)) return -1;
    if (m->probe_mod != i || m->probe_B != B) { ishara_set_error("%s: call ishara_debug_module_forward(training=1) of the head (module %d) with batch %d first", fn, i, B); return -1; }
    if (!logits || !labels) { ishara_set_error("%s: null logits / labels", fn); return -1; }
    m->s = (hipStream_t)st;
    Run r{B, B * m->T, 1, m->probe_seed};
    float* nl = nll ? nll : m->Wf(m->nllb);
    CK(probe_backward_begin(m));
    CKP(m, "ctc", 2.0 * r.M * m->C * 4, 0, launch_ctc(logits, labels, B, m->T, m->C, m->L, m->C - 1, nl, m->Wf(m->dlogits), loss_scale / (float)B, m->Wf(m->ctcws), m->s, m->cls_pad ? m->W(m->dlb) : nullptr));
    if (loss) CKP(m, "mean", 0, 0, launch_mean(nl, loss, B, 1.f / (float)B, m->s));
    void* g = m->W(m->gA);
    CK(head_bwd(m, r, m->W(v[i].in), g));
    CK(wgrad_flush(m));
    CK(red_flush(m));
    if (dx) CK(r5_to_f32(m->dt, g, dx, (size_t)r.M * m->d, m->s));
    return 0;
}
