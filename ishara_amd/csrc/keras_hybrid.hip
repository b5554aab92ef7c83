// The Keras get_model hybrid family, part 2 (graph and workspace plan: keras_graph.hip; Conv1DBlock: conv_block.hip): the other modules, stem, head and
// classifier routes, and ishara_forward / ishara_loss_backward over the kernels in gemm_nt.hip, gemm_tn.hip, norm_rows.hip, dwconv.hip, bn_gate.hip, attention.hip
// and ctc.hip.  confconv_fwd / _bwd also serve the torch families, ln_as_prologue and classifier_fwd the operator entry points (api_ops.hip).
#include "model_types.h"

__global__ void droppath_kernel(float* rs, int B, DropSpec d) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) rs[b] = (d.thr == 0u || rng_keep(rng_row_key(d.key, (uint32_t)b), 0u, d.thr)) ? d.scale : 0.f;
}

// Whether the GEMM [M,K] x [K,N] (weight shadow row stride ldt) applies the LayerNorm in front of it as an operand prologue of the
// A-stationary kernel; if so the prologue fields of ea are set (side outputs mean / rstd / xn: training only, nullptr at inference).
// false: the caller runs layernorm_fwd first.  ishara_forward (ln_prologue) and ishara_op_qkv_fwd both decide here.
bool ln_as_prologue(int dt, int M, int N, int K, int ldt, const float* gamma, const float* beta, float eps, float* mean, float* rstd, void* xn, EpiArgs& ea) {
    EpiArgs probe = ea;
    probe.ln_gamma = gamma; probe.ln_beta = beta; probe.ln_mean = mean; probe.pro_out = xn;
    if (!gemm_nt_as_prologue_ok(dt, dt, dt, M, N, K, ldt, probe)) return false;
    ea.ln_gamma = gamma; ea.ln_beta = beta; ea.ln_eps = eps;
    ea.ln_mean = mean; ea.ln_rstd = rstd; ea.pro_out = xn;
    return true;
}

// LayerNorm as a prologue of the GEMM that consumes it (gemm_as.hip): the wave holds whole rows of K, so the statistics cost two
// cross-lane adds; the normalised rows go to `xn` (training: the weight-gradient GEMM reads them) and the statistics to mean / rstd.
// Shapes the A-stationary kernel does not take run the separate LayerNorm kernel.  Returns the GEMM's A operand.
static const void* ln_prologue(ishara_model* m, const DenseW& w, const Run& r, const void* x, const Norm& ln, float eps, Buf xn, Buf mean, Buf rstd, EpiArgs& ea, int* rc) {
    *rc = 0;
    if (ln_as_prologue(m->dt, r.M, w.N, w.K, w.ldt, m->P(ln.gamma), m->P(ln.beta), eps, r.training ? m->Wf(mean) : nullptr, r.training ? m->Wf(rstd) : nullptr,
                       r.training ? m->W(xn) : nullptr, ea))      // inference: no side outputs
        return x;
    *rc = [&]() -> int {
        CKP(m, "layernorm_fwd", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_layernorm_fwd(m->dt, x, m->P(ln.gamma), m->P(ln.beta), eps, m->W(xn), m->Wf(mean), m->Wf(rstd), r.M, m->d, m->s));
        return 0;
    }();
    return m->W(xn);
}

// ------------------------------------------------------------------ module forward
int ffn_fwd(ishara_model* m, FFN& f, const Run& r, const void* x) {
    const int dt = m->dt;
    OpArgs no;
    EpiArgs ea; ea.pre_out = m->W(f.za); ea.act = ACT_SWISH; ea.drop = dspec(r, f.site_in, m->cfg.dropout_rate);
    int rc;
    const void* ain = ln_prologue(m, f.Wa, r, x, f.ln, f.eps, f.xn, f.mean, f.rstd, ea, &rc);
    CK(rc);
    CK(gemm_fwd(m, f.Wa, ain, dt, m->W(f.u), dt, r.M, OP_NONE, no, ea));
    EpiArgs eb; eb.resid = x;
    if (f.has_out_drop) eb.drop = dspec(r, f.site_out, m->cfg.dropout_rate);
    CK(gemm_fwd(m, f.Wb, m->W(f.u), dt, m->W(f.out), dt, r.M, OP_NONE, no, eb));
    return 0;
}

int mhsa_fwd(ishara_model* m, MHSA& a, const Run& r, const void* x) {
    const int dt = m->dt;
    OpArgs no;
    EpiArgs eq; eq.mode = EPI_QKV; eq.q = m->W(a.q); eq.k = m->W(a.k); eq.vt = m->W(a.vt); eq.H = m->H; eq.dh = m->dh; eq.T = m->T; eq.head_major = 1;
    int rc;
    const void* ain = ln_prologue(m, a.Wqkv, r, x, a.ln, a.eps, a.xn, a.mean, a.rstd, eq, &rc);
    CK(rc);
    CK(gemm_fwd(m, a.Wqkv, ain, dt, nullptr, dt, r.M, OP_NONE, no, eq));
    const float scale = 1.0f / sqrtf((float)m->d);     // self.scale = dim ** -0.5 (c5:95)
    CKP(m, "attn_fwd", 4.0 * r.M * m->d * (double)dt_size(m->dt), 4.0 * r.B * m->H * (double)m->T * m->T * m->dh, launch_attn_fwd(dt, m->W(a.q), m->W(a.k), m->W(a.vt), m->W(a.o), m->Wf(a.lse), r.B, m->H, m->T, m->dh, scale,
                       dspec_attn(r, a.site_attn, a.rate), m->cfg.attn_impl, reinterpret_cast<uint32_t*>(m->W(a.maskw)), m->s, nullptr, r.key_len));      // frame lengths: keys j >= n_b excluded (c5:109-112)
    EpiArgs ep; ep.resid = x;
    if (a.has_out_drop) ep.drop = dspec(r, a.site_out, m->cfg.dropout_rate);
    CK(gemm_fwd(m, a.Wp, m->W(a.o), dt, m->W(a.out), dt, r.M, OP_NONE, no, ep));
    return 0;
}

int sqzconv_fwd(ishara_model* m, SqzConv& c, const Run& r, const void* x) {
    const int dt = m->dt, d = m->d, de = c.Wc1.N, B = r.B, T = m->T;
    OpArgs no; EpiArgs e0;
    EpiArgs e1;
    int rc;
    const void* ain = ln_prologue(m, c.Wc1, r, x, c.ln, 1e-6f, c.xn, c.mean, c.rstd, e1, &rc);
    CK(rc);
    CK(gemm_fwd(m, c.Wc1, ain, dt, m->W(c.zc), dt, r.M, OP_NONE, no, e1));
    CKP(m, "dwconv_fwd", 3.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_dwconv_fwd(dt, DWIN_SWISH, m->W(c.zc), m->P(c.dw), nullptr, m->W(c.zd), nullptr, nullptr, nullptr, B, T, de, c.k, c.k - 1, m->s));
    CKP(m, "map_rows", 2.0 * r.M * de * (double)dt_size(m->dt), 0, launch_map_rows(dt, MAP_SWISH, m->W(c.zd), m->W(c.hd), nullptr, DropSpec{0, 0, 1.f}, r.M, T, de, m->s));
    CK(gemm_fwd(m, c.Wc3, m->W(c.hd), dt, m->W(c.u3), dt, r.M, OP_NONE, no, e0));
    // frame lengths: z = mean of u3 over the valid frames (c5:129-130): c.gap holds the masked mean, the SE kernels run with invT = 1
    if (r.key_len) CKP(m, "masked_time_mean", 1.0 * r.M * d * (double)dt_size(dt), 0, launch_masked_time_mean(dt, m->W(c.u3), r.key_len, m->Wf(c.gap), B, T, d, m->s));
    else
    CKP(m, "sample_reduce", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_reduce(dt, m->W(c.u3), nullptr, nullptr, nullptr, m->Wf(c.gap), nullptr, B, T, d, m->s));
    CKP(m, "se_fwd", 0, 0, launch_se_fwd(m->Wf(c.gap), r.key_len ? 1.f : 1.f / T, m->P(c.seW1), m->P(c.seb1), m->P(c.seW2), m->P(c.seb2), m->Wf(c.hid), m->Wf(c.se), B, d, c.R, m->s));
    CKP(m, "sample_affine", 4.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_affine(dt, m->W(c.u3), m->Wf(c.se), nullptr, x, m->W(c.out), B, T, d, m->s));
    return 0;
}

int confconv_fwd(ishara_model* m, ConfConv& c, const Run& r, const void* x) {
    const int dt = m->dt, d = m->d, B = r.B, T = m->T;
    OpArgs no; EpiArgs e0;
    CK(gemm_fwd(m, c.Wp1, x, dt, m->W(c.g), dt, r.M, OP_NONE, no, e0));
    const float var_corr = c.bn_unbiased && B * T > 1 ? (float)((double)B * T / ((double)B * T - 1.0)) : 1.f;
    const DwBnFwd st = {c.bn, c.bn_eps, c.bn_keep, var_corr, c.ssum, c.ssq, c.mean, c.rstd, c.a, c.bsh};
    // training: batch statistics straight from the depthwise conv's partial rows (no stats_reduce launch); inference: no batch statistics at all
    const int prows = r.training && stats_fusion_on() ? dwconv_stat_rows(dt, B, T, d, c.k) : 0;
    CK(dwconv_bn_fwd(m, r, DWIN_GLU, m->W(c.g), c.dw, c.dwb, m->W(c.v), d, c.k, (c.k - 1) / 2, st, r.training != 0, prows, true));
    CKP(m, "col_affine", 2.0 * r.M * d * (double)dt_size(m->dt), 0, launch_col_affine(dt, m->W(c.v), m->Wf(c.a), m->Wf(c.bsh), m->W(c.bnv), r.M, d, m->s));
    const void* pin = m->W(c.bnv);
    if (c.swish_after_bn) {
        CKP(m, "map_rows", 2.0 * r.M * d * (double)dt_size(m->dt), 0, launch_map_rows(dt, MAP_SWISH, m->W(c.bnv), m->W(c.sw), nullptr, DropSpec{0, 0, 1.f}, r.M, T, d, m->s));
        pin = m->W(c.sw);
    }
    EpiArgs e2; e2.resid = x;
    if (c.has_out_drop) e2.drop = dspec(r, c.site_out, m->cfg.dropout_rate);
    CK(gemm_fwd(m, c.Wp2, pin, dt, m->W(c.r), dt, r.M, OP_NONE, no, e2));
    CKP(m, "layernorm_fwd", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_layernorm_fwd(dt, m->W(c.r), m->P(c.ln.gamma), m->P(c.ln.beta), c.ln_eps, m->W(c.out), m->Wf(c.lnmean), m->Wf(c.lnrstd), r.M, d, m->s));
    return 0;
}

// ---- the classifier Dense of the head: fp32 logits [M, C] from A [M, K] (dt) and the weight shadow Wt (rows of ldt elements, at least
// 64 rows, zero-filled beyond C).  ishara_forward and ishara_op_classifier_fwd both run it here.
//   CLS_AS      the A-stationary MFMA kernel over N = 64 shadow rows, storing the C real columns only (ldc = n_valid = C)
//   CLS_NARROW  dense_narrow (one lane per class)
//   CLS_GEMM    the NT GEMM with fp32 output (launch_gemm_nt picks the kernel)
//   CLS_AUTO    what the model takes for (dt, M, K, C): CLS_AS for 16-bit dt, M <= 1536, C <= 64, C % 4 == 0, K 256 / 512; else CLS_NARROW
//               for 16-bit dt, M <= 4096, C <= 64, K % 32 == 0; else CLS_GEMM.  ISHARA_NO_INFER_FUSION or a forced tile kernel
//               (ishara_debug_force_regstage) rule out CLS_AS, the former CLS_NARROW too.
int cls_route_auto(int dt, int M, int K, int C) {
    const bool fusion = infer_fusion_on();
    if (dt_is16(dt) && M <= 1536 && C <= 64 && C % 4 == 0 && (K == 256 || K == 512) && !g_force_regstage && fusion) return CLS_AS;      // a clip's worth of rows
    if (dt_is16(dt) && M <= 4096 && C <= 64 && K % 32 == 0 && fusion) return CLS_NARROW;      // few rows: the latency of a clip
    return CLS_GEMM;
}
// m: the model whose profiler records the launch (nullptr: none)
#define CKP_OPT(m, key, by, fl, expr) do { if (m) CKP(m, key, by, fl, expr); else CK(expr); } while (0)
int classifier_fwd(ishara_model* m, int route, int dt, const void* A, const void* Wt, int ldt, const float* bias, float* logits, int M, int K, int C, hipStream_t s) {
    if (route == CLS_AUTO) route = cls_route_auto(dt, M, K, C);
    OpArgs no; EpiArgs ec; ec.bias = bias;
    if (route == CLS_AS) {
        ec.ldc = C; ec.n_valid = C;
        CKP_OPT(m, "classifier(as)", 0, 2.0 * M * C * K, launch_gemm_nt(dt, dt, DT_F32, OP_NONE, A, Wt, logits, M, 64, K, ldt, no, ec, s));
    } else if (route == CLS_NARROW) {
        CKP_OPT(m, "dense_narrow", 0, 2.0 * M * C * K, launch_dense_narrow(dt, A, Wt, ldt, bias, logits, M, C, K, s));
    } else {
        const double by = (double)M * K * dt_size(dt) + (double)M * C * 4 + (double)K * C * dt_size(dt);
        CKP_OPT(m, gemm_nt_kernel_name(dt, dt, DT_F32, OP_NONE, A, M, C, K, ldt, ec), by, 2.0 * M * C * K, launch_gemm_nt(dt, dt, DT_F32, OP_NONE, A, Wt, logits, M, C, K, ldt, no, ec, s));
    }
    return 0;
}

// stem and head of the sequential graph: ishara_forward / ishara_loss_backward and the module probe (ishara_debug_module_*) both run them here
int stem_fwd(ishara_model* m, const Run& r, const float* x) {
    const int dt = m->dt, d = m->d, T = m->T, B = r.B, training = r.training;
    OpArgs no;
    // ---- stem: Dense(no bias) + PE, BatchNorm(momentum .95)  (c7:13-17)
    EpiArgs es; es.addtab = m->Wf(m->pe); es.tab_period = T;
    if (m->stem_kp) {       // bf16: pack the input rows once, then the Dense (and its wgrad) run on the bf16 fast paths with K = stem_kp
        CKP(m, "pack_rows_bf16", (double)r.M * (m->F * 4.0 + m->stem_kp * 2.0), 0, launch_pack_rows_bf16(x, m->W(m->stem_xb), r.M, m->F, m->stem_kp, m->s, dt));
        DenseW wp = m->stemW; wp.K = m->stem_kp;
        CK(gemm_fwd(m, wp, m->W(m->stem_xb), dt, m->W(m->stem_h0), dt, r.M, OP_NONE, no, es));
    } else
        CK(gemm_fwd(m, m->stemW, x, DT_F32, m->W(m->stem_h0), dt, r.M, OP_NONE, no, es));
    if (training)           // (inference: the BatchNorm uses its moving statistics, nothing reads the batch sums)
    CKP(m, "sample_reduce", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_reduce(dt, m->W(m->stem_h0), m->W(m->stem_h0), nullptr, nullptr, m->Wf(m->stem_ssum), m->Wf(m->stem_ssq), B, T, d, m->s));
    CKP(m, "bn_finalize", 0, 0, launch_bn_finalize(m->Wf(m->stem_ssum), m->Wf(m->stem_ssq), B, (float)B * T, m->P(m->stem_bn.gamma), m->P(m->stem_bn.beta), 1e-3f, 0.95f,
                          m->P(m->stem_bn.mm), m->P(m->stem_bn.mv), training, m->Wf(m->stem_mean), m->Wf(m->stem_rstd), m->Wf(m->stem_a), m->Wf(m->stem_bsh), d, m->s));
    CKP(m, "col_affine", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_col_affine(dt, m->W(m->stem_h0), m->Wf(m->stem_a), m->Wf(m->stem_bsh), m->W(m->stem_out), r.M, d, m->s));
    return 0;
}
int head_fwd(ishara_model* m, const Run& r, const void* h, float* logits) {
    const int dt = m->dt;
    OpArgs no;
    // ---- head: Dense(relu) -> Dropout(0.4) -> Dense  (c7:61-63)
    EpiArgs et; et.act = ACT_RELU; et.drop = dspec(r, m->head_site, m->cfg.head_dropout);
    CK(gemm_fwd(m, m->topW, h, dt, m->W(m->head_hh), dt, r.M, OP_NONE, no, et));
    CK(classifier_fwd(m, CLS_AUTO, dt, m->W(m->head_hh), m->ws + m->clsW.wt, m->clsW.ldt, m->clsW.b >= 0 ? m->P(m->clsW.b) : nullptr, logits, r.M, m->clsW.K, m->C, m->s));
    return 0;
}

// what every entry point that takes frame lengths refuses before any GPU work (frame_len == NULL: nothing to refuse)
bool frame_len_ok(const ishara_model* m, const char* fn, const int32_t* frame_len) {
    if (!frame_len) return true;
    if (m->family != ISHARA_FAMILY_KERAS_HYBRID) { ishara_set_error("%s: frame lengths are for ISHARA_FAMILY_KERAS_HYBRID only (family %d)", fn, m->family); return false; }
    if (m->dt == DT_F16) { ishara_set_error("%s: ISHARA_F16 takes no frame lengths (the fp16 model is the TFLite export, whose graph has no mask)", fn); return false; }
    if ((uintptr_t)frame_len % 4 != 0) { ishara_set_error("%s: frame_len must be 4-byte aligned", fn); return false; }
    return true;
}
static int keras_forward(const char* fn, ishara_model* m, const float* x, int32_t B, float* logits, int32_t training, uint32_t seed, const int32_t* frame_len, ishara_stream st) {
    if (!frame_len_ok(m, fn, frame_len)) return -1;      // (with lengths: family, storage type and alignment before anything else)
    if (!m->ws) { ishara_set_error("%s: model is not bound", fn); return -1; }
    if (m->family != ISHARA_FAMILY_KERAS_HYBRID) { ishara_set_error("%s: this handle is an encoder-only family; use ishara_encoder_forward", fn); return -1; }
    if (B <= 0 || B > m->Bmax) { ishara_set_error("%s: batch %d outside 1..%d", fn, B, m->Bmax); return -1; }
    if (m->dt == DT_F16 && training) {
        ishara_set_error("%s: ISHARA_F16 is an inference-only storage type (the reference's fp16 is the TFLite export, c14:1-5; it reports NaNs when TRAINING in fp16)", fn);
        return -1;
    }
    m->s = (hipStream_t)st;
    Run r{B, B * m->T, training, seed};
    r.key_len = frame_len;
    CK(stem_fwd(m, r, x));
    const void* h = m->W(m->stem_out);
    for (const Layer& L : m->layers) {
        if (L.kind == Layer::CONV) { ConvBlock& cb = m->convs[L.idx]; CK(conv_fwd(m, cb, r, h)); h = m->W(cb.out); }
        else if (L.kind == Layer::SQZ) {
            SqzBlock& sb = m->sqz[L.idx];
            CK(ffn_fwd(m, sb.ffn1, r, h)); h = m->W(sb.ffn1.out);
            CK(mhsa_fwd(m, sb.mha, r, h)); h = m->W(sb.mha.out);
            CK(sqzconv_fwd(m, sb.conv, r, h)); h = m->W(sb.conv.out);
            CK(ffn_fwd(m, sb.ffn2, r, h)); h = m->W(sb.ffn2.out);
        } else {
            ConfBlock& cb = m->conf[L.idx];
            CK(ffn_fwd(m, cb.ffn1, r, h)); h = m->W(cb.ffn1.out);
            CK(mhsa_fwd(m, cb.mha, r, h)); h = m->W(cb.mha.out);
            CK(confconv_fwd(m, cb.conv, r, h)); h = m->W(cb.conv.out);
            CK(ffn_fwd(m, cb.ffn2, r, h)); h = m->W(cb.ffn2.out);
        }
    }
    CK(head_fwd(m, r, h, logits));
    m->lastB = B; m->last_training = training; m->last_seed = seed; m->last_x = x; m->probe_mod = -1; m->last_masked = frame_len ? 1 : 0;
    return 0;
}
extern "C" int ishara_forward(ishara_model* m, const float* x, int32_t B, float* logits, int32_t training, uint32_t seed, ishara_stream st) {
    return keras_forward("ishara_forward", m, x, B, logits, training, seed, nullptr, st);
}
extern "C" int ishara_forward_ex(ishara_model* m, const float* x, int32_t B, float* logits, int32_t training, uint32_t seed, const int32_t* frame_len, ishara_stream st) {
    return keras_forward("ishara_forward_ex", m, x, B, logits, training, seed, frame_len, st);
}

// ------------------------------------------------------------------ module backward: each *_bwd consumes g (grad wrt the module output) and writes gn (grad wrt its input x)
static const void* layer_out(ishara_model* m, const Layer& L) {      // output activation of a layer of the sequential graph
    return L.kind == Layer::CONV ? m->W(m->convs[L.idx].out) : (L.kind == Layer::SQZ ? m->W(m->sqz[L.idx].ffn2.out) : m->W(m->conf[L.idx].ffn2.out));
}

int ffn_bwd(ishara_model* m, FFN& f, const Run& r, const void* x, const void* g, void* gn) {
    const int dt = m->dt;
    OpArgs no;
    int rc = 0;
    const void* gs = f.has_out_drop ? grad_through_dropout(m, r, f.site_out, m->cfg.dropout_rate, g, m->W(m->t3), m->T, m->d, &rc) : g;      // the outer dropout
    CK(rc);
    EpiArgs e1; e1.drop = dspec(r, f.site_in, m->cfg.dropout_rate); e1.dact = DACT_SWISH; e1.aux = m->W(f.za);
    CK(gemm_dgrad(m, f.Wb, gs, dt, m->W(m->t1), r.M, OP_NONE, no, e1));                         // dza
    CK(gemm_wgrad(m, f.Wb, m->W(f.u), dt, OP_NONE, no, gs, dt, OP_NONE, no, r.M));
    EpiArgs e0;
    CK(gemm_dgrad(m, f.Wa, m->W(m->t1), dt, m->W(m->t2), r.M, OP_NONE, no, e0));              // dxn
    CK(gemm_wgrad(m, f.Wa, m->W(f.xn), dt, OP_NONE, no, m->W(m->t1), dt, OP_NONE, no, r.M));
    return layernorm_bwd_deferred(m, r, m->W(m->t2), x, f.mean, f.rstd, f.ln, g, gn);
}

int mhsa_bwd(ishara_model* m, MHSA& a, const Run& r, const void* x, const void* g, void* gn) {
    const int dt = m->dt;
    OpArgs no; EpiArgs e0;
    int rc = 0;
    const void* gs = a.has_out_drop ? grad_through_dropout(m, r, a.site_out, m->cfg.dropout_rate, g, m->W(m->t3), m->T, m->d, &rc) : g;
    CK(rc);
    CK(gemm_dgrad(m, a.Wp, gs, dt, m->W(m->t1), r.M, OP_NONE, no, e0));                         // do
    CK(gemm_wgrad(m, a.Wp, m->W(a.o), dt, OP_NONE, no, gs, dt, OP_NONE, no, r.M));
    const float scale = 1.0f / sqrtf((float)m->d);
    CKP(m, "attn_bwd", 8.0 * r.M * m->d * (double)dt_size(m->dt), 10.0 * r.B * m->H * (double)m->T * m->T * m->dh, launch_attn_bwd(dt, m->W(a.q), m->W(a.k), m->W(a.vt), m->W(a.o), m->W(m->t1), m->Wf(a.lse), m->Wf(m->delta), m->W(m->t2),
                       r.B, m->H, m->T, m->dh, scale, dspec_attn(r, a.site_attn, a.rate), 1, m->cfg.attn_impl, reinterpret_cast<uint32_t*>(m->W(a.maskw)), m->s, nullptr, r.key_len));
    CK(gemm_dgrad(m, a.Wqkv, m->W(m->t2), dt, m->W(m->t1), r.M, OP_NONE, no, e0));            // dxn
    CK(gemm_wgrad(m, a.Wqkv, m->W(a.xn), dt, OP_NONE, no, m->W(m->t2), dt, OP_NONE, no, r.M));
    return layernorm_bwd_deferred(m, r, m->W(m->t1), x, a.mean, a.rstd, a.ln, g, gn);
}

int sqzconv_bwd(ishara_model* m, SqzConv& c, const Run& r, const void* x, const void* g, void* gn) {
    const int dt = m->dt, d = m->d, de = c.Wc1.N, B = r.B, T = m->T;
    OpArgs no; EpiArgs e0;
    CKP(m, "sample_reduce", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_reduce(dt, g, m->W(c.u3), nullptr, nullptr, m->Wf(m->S1), m->Wf(m->dse), B, T, d, m->s));   // dse = sum_t g*u3
    CKP(m, "se_bwd", 0, 0, launch_se_bwd(m->Wf(m->dse), m->Wf(c.gap), r.key_len ? 1.f : 1.f / T, m->P(c.seW1), m->P(c.seW2), m->Wf(c.hid), m->Wf(c.se),
                     m->G(c.seW1), m->G(c.seb1), m->G(c.seW2), m->G(c.seb2), m->Wf(m->dgapT), m->Wf(m->E), B, d, c.R, m->s));
    if (r.key_len)      // frame lengths: c.gap is the masked mean, dgapT its gradient; dgapT / n_b goes to the valid frames only
    CKP(m, "sample_affine_len", 4.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_affine_len(dt, g, m->Wf(c.se), m->Wf(m->dgapT), r.key_len, m->W(m->t1), B, T, d, m->s));
    else
    CKP(m, "sample_affine", 4.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_affine(dt, g, m->Wf(c.se), m->Wf(m->dgapT), nullptr, m->W(m->t1), B, T, d, m->s));           // du3
    EpiArgs e1; e1.dact = DACT_SWISH; e1.aux = m->W(c.zd);
    CK(gemm_dgrad(m, c.Wc3, m->W(m->t1), dt, m->W(m->t2), r.M, OP_NONE, no, e1));                                // dzd
    CK(gemm_wgrad(m, c.Wc3, m->W(c.hd), dt, OP_NONE, no, m->W(m->t1), dt, OP_NONE, no, r.M));
    CK(dwconv_bwd_deferred(m, r, 8.0, DWIN_SWISH, m->W(m->t2), nullptr, m->W(c.zc), c.dw, -1, m->W(m->t1), de, c.k, c.k - 1));   // dzc
    CK(gemm_dgrad(m, c.Wc1, m->W(m->t1), dt, m->W(m->t2), r.M, OP_NONE, no, e0));                                // dxn
    CK(gemm_wgrad(m, c.Wc1, m->W(c.xn), dt, OP_NONE, no, m->W(m->t1), dt, OP_NONE, no, r.M));
    return layernorm_bwd_deferred(m, r, m->W(m->t2), x, c.mean, c.rstd, c.ln, g, gn);
}

int confconv_bwd(ishara_model* m, ConfConv& c, const Run& r, const void* x, const void* g, void* gn) {
    const int dt = m->dt, d = m->d, B = r.B, T = m->T;
    OpArgs no;
    CK(layernorm_bwd_deferred(m, r, g, m->W(c.r), c.lnmean, c.lnrstd, c.ln, nullptr, m->W(m->t1)));   // dr
    int rc = 0;
    const void* gs = c.has_out_drop ? grad_through_dropout(m, r, c.site_out, m->cfg.dropout_rate, m->W(m->t1), m->W(m->t3), T, d, &rc) : m->W(m->t1);      // the module's output dropout
    CK(rc);
    EpiArgs es; if (c.swish_after_bn) { es.dact = DACT_SWISH; es.aux = m->W(c.bnv); }
    CK(gemm_dgrad(m, c.Wp2, gs, dt, m->W(m->t2), r.M, OP_NONE, no, es));                                          // d bn(v)
    CK(gemm_wgrad(m, c.Wp2, c.swish_after_bn ? m->W(c.sw) : m->W(c.bnv), dt, OP_NONE, no, gs, dt, OP_NONE, no, r.M));
    CKP(m, "sample_reduce", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_reduce(dt, m->W(m->t2), m->W(c.v), m->Wf(c.mean), m->Wf(c.rstd), m->Wf(m->S1), m->Wf(m->S2), B, T, d, m->s));
    CKP(m, "bn_bwd_finalize", 0, 0, launch_bn_bwd_finalize(m->Wf(m->S1), m->Wf(m->S2), m->G(c.bn.gamma), m->G(c.bn.beta), m->Wf(m->Ecol), m->Wf(m->Fc), B, T, d, m->s));
    DwBnArgs bn; bn.h = m->W(c.v); bn.mean = m->Wf(c.mean); bn.rstd = m->Wf(c.rstd); bn.a = m->Wf(c.a); bn.E = m->Wf(m->Ecol); bn.Fc = m->Wf(m->Fc);
    CK(dwconv_bn_bwd(m, r, dwconv_bwd_fused_bn(dt, d, c.k, (c.k - 1) / 2), 6.0, DWIN_GLU, m->W(m->t2), bn, m->W(c.g), c.dw, c.dwb, m->W(m->t3), d, c.k, (c.k - 1) / 2));   // dv in place where not fused; dg [M,2d]
    EpiArgs e2; e2.resid = m->W(m->t1);
    CK(gemm_dgrad(m, c.Wp1, m->W(m->t3), dt, gn, r.M, OP_NONE, no, e2));
    CK(gemm_wgrad(m, c.Wp1, x, dt, OP_NONE, no, m->W(m->t3), dt, OP_NONE, no, r.M));
    return 0;
}

// head backward: g = gradient with respect to the head's input hin, from dlogits / dlb (the CTC kernel wrote them)
int head_bwd(ishara_model* m, const Run& r, const void* hin, void* g) {
    const int dt = m->dt;
    OpArgs no; EpiArgs e0;
    EpiArgs eh; eh.drop = dspec(r, m->head_site, m->cfg.head_dropout); eh.dact = DACT_POS; eh.aux = m->W(m->head_hh);
    if (m->cls_pad && r.M % 64 == 0 && r.M >= 256 && m->clsW.K % 128 == 0 && !g_force_tn_regstage) {
        DenseW wp = m->clsW; wp.N = m->cls_pad;          // reduction / output width of the padded operand; the real classes are the first m->C
        CK(gemm_dgrad(m, wp, m->W(m->dlb), dt, m->W(m->t1), r.M, OP_NONE, no, eh));
        CK(gemm_wgrad(m, wp, m->W(m->head_hh), dt, OP_NONE, no, m->W(m->dlb), dt, OP_NONE, no, r.M, 0, m->C));
    } else {
        CK(gemm_dgrad(m, m->clsW, m->Wf(m->dlogits), DT_F32, m->W(m->t1), r.M, OP_NONE, no, eh));
        CK(gemm_wgrad(m, m->clsW, m->W(m->head_hh), dt, OP_NONE, no, m->Wf(m->dlogits), DT_F32, OP_NONE, no, r.M));
    }
    CK(gemm_dgrad(m, m->topW, m->W(m->t1), dt, g, r.M, OP_NONE, no, e0));
    CK(gemm_wgrad(m, m->topW, hin, dt, OP_NONE, no, m->W(m->t1), dt, OP_NONE, no, r.M));
    return 0;
}
// stem backward: parameter gradients from g, the gradient with respect to the stem's output
int stem_bwd(ishara_model* m, const Run& r, const void* g) {
    const int dt = m->dt, d = m->d, T = m->T, B = r.B;
    OpArgs no;
    CKP(m, "sample_reduce", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_reduce(dt, g, m->W(m->stem_h0), m->Wf(m->stem_mean), m->Wf(m->stem_rstd), m->Wf(m->S1), m->Wf(m->S2), B, T, d, m->s));
    CKP(m, "bn_bwd_finalize", 0, 0, launch_bn_bwd_finalize(m->Wf(m->S1), m->Wf(m->S2), m->G(m->stem_bn.gamma), m->G(m->stem_bn.beta), m->Wf(m->Ecol), m->Wf(m->Fc), B, T, d, m->s));
    CKP(m, "bn_bwd_apply", 6.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_bn_bwd_apply(dt, g, m->W(m->stem_h0), m->Wf(m->stem_mean), m->Wf(m->stem_rstd), m->Wf(m->stem_a), nullptr, m->Wf(m->Ecol), 0, m->Wf(m->Fc), m->W(m->t1), B, T, d, m->s));
    if (m->stem_kp && r.M % 64 == 0 && r.M >= 256 && d % 128 == 0 && !g_force_tn_regstage) {
        DenseW wp = m->stemW; wp.K = m->stem_kp;           // packed rows of the forward pass; only the first F rows of dW exist
        CK(gemm_wgrad(m, wp, m->W(m->stem_xb), dt, OP_NONE, no, m->W(m->t1), dt, OP_NONE, no, r.M, m->F));
    } else
        CK(gemm_wgrad(m, m->stemW, m->last_x, DT_F32, OP_NONE, no, m->W(m->t1), dt, OP_NONE, no, r.M));
    return 0;
}

// a backward call must be given frame lengths exactly when its training forward was (the arrays are the caller's: only that bit is kept)
bool frame_len_agrees(const char* fn, bool fwd_had, const int32_t* frame_len) {
    if (fwd_had == (frame_len != nullptr)) return true;
    ishara_set_error("%s: the training forward was %s frame lengths, this call is %s", fn, fwd_had ? "given" : "not given", frame_len ? "given some" : "given none");
    return false;
}
// A second loss term between the CTC kernel and the head: the gradient of risk_scale / B * sum_n coef[b, n] * nll_n over an n-best list, added
// into m->dlogits (and m->dlb rewritten from the sum) by ishara_ctc_nbest_grad's kernels.  nullptr: no stage, the launches of before.
// A third term behind it, of the same shape: kd (the public ishara_kd_stage), the distillation gradient kd_scale / B * (w_b * (ps - pt)) by
// ishara_kd_grad's kernels.  nullptr: no stage.
struct NbestStage { const int32_t* hyp_idx; const int32_t* hyp_len; int32_t N, Th, max_len; const float* coef; float risk_scale; void* ws; };
static int keras_loss_backward(const char* fn, ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale, const int32_t* frame_len, ishara_stream st,
                               const NbestStage* nb = nullptr, const ishara_kd_stage* kd = nullptr) {
    if (!frame_len_ok(m, fn, frame_len)) return -1;
    if (!m->ws || !m->grads) { ishara_set_error("%s: model is not bound (grads required)", fn); return -1; }
    if (m->family != ISHARA_FAMILY_KERAS_HYBRID) { ishara_set_error("%s: this handle is an encoder-only family; use ishara_encoder_backward", fn); return -1; }
    if (B != m->lastB || !m->last_training) { ishara_set_error("%s: call ishara_forward(training=1) with the same batch first", fn); return -1; }
    if (!frame_len_agrees(fn, m->last_masked != 0, frame_len)) return -1;
    m->s = (hipStream_t)st;
    m->red.njobs = 0; m->red.nblocks = 0; m->red_off = 0; g_red_sink = nullptr;       // ... nor recorded column sums
    m->tn_defer.pending = false;        // a previous backward pass that returned early (error path) must not leave slab sums behind for this one to add
    Run r{B, B * m->T, 1, m->last_seed};
    r.key_len = frame_len;      // the three masked operations only: the CTC loss below keeps logit_length = T (c6:3)
    const int T = m->T;
    float* nl = nll ? nll : m->Wf(m->nllb);
    CK(launch_fill_u32(m->grads, (size_t)m->n_train, 0u, m->s));      // a kernel, not a memset node: the whole step stays capturable (hipGraph note)
    CKP(m, "ctc", 2.0 * r.M * m->C * 4, 0, launch_ctc(logits, labels, B, T, m->C, m->L, m->C - 1, nl, m->Wf(m->dlogits), loss_scale / (float)B, m->Wf(m->ctcws), m->s, m->cls_pad ? m->W(m->dlb) : nullptr));
    if (loss) CKP(m, "mean", 0, 0, launch_mean(nl, loss, B, 1.f / (float)B, m->s));
    if (nb)     // the risk term keeps logit_length = T, as the CTC loss above
        CKP(m, "ctc_nbest_grad", 2.0 * r.M * m->C * 4, 0, launch_ctc_nbest_grad(logits, B, T, m->C, m->C - 1, nb->hyp_idx, nb->hyp_len, nb->N, nb->Th, nb->max_len, nullptr, nb->coef,
                                                                                  nb->risk_scale / (float)B, m->Wf(m->dlogits), 1, m->cls_pad ? m->W(m->dlb) : nullptr, nullptr, nullptr, nb->ws, m->s));
    if (kd)     // the distillation term behind it, with logit_length = T as well; the stage that runs last leaves m->dlb
        CKP(m, "kd_grad", 4.0 * r.M * m->C * 4, 0, launch_kd_grad(logits, kd->teacher, B, T, m->C, kd->inv_temp, kd->mode, nullptr, kd->kd_scale / (float)B, m->Wf(m->dlogits), 1,
                                                                  m->cls_pad ? m->W(m->dlb) : nullptr, kd->kl_frame, kd->kl_clip, m->s));
    // ---- head
    // input of the head = output of the last layer
    const void* hin = m->layers.empty() ? m->W(m->stem_out) : layer_out(m, m->layers.back());
    void* g = m->W(m->gA); void* gn = m->W(m->gB);
    CK(head_bwd(m, r, hin, g));
    // ---- layers in reverse; `in_of` = input activation of each module
    for (int li = (int)m->layers.size() - 1; li >= 0; --li) {
        const Layer& L = m->layers[li];
        const void* lin = li > 0 ? layer_out(m, m->layers[li - 1]) : m->W(m->stem_out);
#define STEP(call) do { CK(call); void* _t = g; g = gn; gn = _t; } while (0)
        if (L.kind == Layer::CONV) { STEP(conv_bwd(m, m->convs[L.idx], r, lin, g, gn)); }
        else if (L.kind == Layer::SQZ) {
            SqzBlock& sb = m->sqz[L.idx];
            STEP(ffn_bwd(m, sb.ffn2, r, m->W(sb.conv.out), g, gn));
            STEP(sqzconv_bwd(m, sb.conv, r, m->W(sb.mha.out), g, gn));
            STEP(mhsa_bwd(m, sb.mha, r, m->W(sb.ffn1.out), g, gn));
            STEP(ffn_bwd(m, sb.ffn1, r, lin, g, gn));
        } else {
            ConfBlock& cb = m->conf[L.idx];
            STEP(ffn_bwd(m, cb.ffn2, r, m->W(cb.conv.out), g, gn));
            STEP(confconv_bwd(m, cb.conv, r, m->W(cb.mha.out), g, gn));
            STEP(mhsa_bwd(m, cb.mha, r, m->W(cb.ffn1.out), g, gn));
            STEP(ffn_bwd(m, cb.ffn1, r, lin, g, gn));
        }
#undef STEP
        if (!m->bucket_ev.empty() && m->bucket_after_layer[li] >= 0) { CK(wgrad_flush(m)); CK(red_flush(m)); HIP_CHECK_RET(hipEventRecord(m->bucket_ev[m->bucket_after_layer[li]], m->s)); }
    }
    // ---- stem
    CK(stem_bwd(m, r, g));
    CK(wgrad_flush(m));
    CK(red_flush(m));
    if (!m->bucket_ev.empty()) HIP_CHECK_RET(hipEventRecord(m->bucket_ev.back(), m->s));
    return 0;
}
extern "C" int ishara_loss_backward(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale, ishara_stream st) {
    return keras_loss_backward("ishara_loss_backward", m, logits, labels, B, loss, nll, loss_scale, nullptr, st);
}
extern "C" int ishara_loss_backward_ex(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale, const int32_t* frame_len,
                                       ishara_stream st) {
    return keras_loss_backward("ishara_loss_backward_ex", m, logits, labels, B, loss, nll, loss_scale, frame_len, st);
}
extern "C" int ishara_loss_backward_nbest(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale,
                                          const int32_t* frame_len, const int32_t* hyp_idx, const int32_t* hyp_len, int32_t N, int32_t Th, int32_t max_len,
                                          const float* coef, float risk_scale, void* workspace, ishara_stream st) {
    const char* fn = "ishara_loss_backward_nbest";
    if (!m) { ishara_set_error("%s: null model", fn); return -1; }
    if (B < 1) { ishara_set_error("%s: B=%d < 1", fn, B); return -1; }
    // the stage's own refusals before anything is launched; dlogits is the model's buffer
    const int rc = ctc_nbest_grad_check(fn, logits, B, m->T, m->C, m->C - 1, hyp_idx, hyp_len, N, Th, max_len, nullptr, coef, m->ws ? m->Wf(m->dlogits) : nullptr, nullptr,
                                        nullptr, nullptr, workspace);
    if (rc != 0) return rc;
    const NbestStage nb{hyp_idx, hyp_len, N, Th, max_len, coef, risk_scale, workspace};
    return keras_loss_backward(fn, m, logits, labels, B, loss, nll, loss_scale, frame_len, st, &nb);
}
extern "C" int ishara_loss_backward_kd(ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale,
                                       const int32_t* frame_len, const ishara_kd_stage* kd, const ishara_nbest_stage* nbest, ishara_stream st) {
    const char* fn = "ishara_loss_backward_kd";
    if (!m) { ishara_set_error("%s: null model", fn); return -1; }
    if (B < 1) { ishara_set_error("%s: B=%d < 1", fn, B); return -1; }
    // both stages' own refusals before anything is launched; dlogits and dlb are the model's buffers
    const float* dl = m->ws ? m->Wf(m->dlogits) : nullptr;
    NbestStage nb{};
    if (nbest) {
        const int rc = ctc_nbest_grad_check(fn, logits, B, m->T, m->C, m->C - 1, nbest->hyp_idx, nbest->hyp_len, nbest->N, nbest->Th, nbest->max_len, nullptr, nbest->coef, dl,
                                            nullptr, nullptr, nullptr, nbest->workspace);
        if (rc != 0) return rc;
        nb = NbestStage{nbest->hyp_idx, nbest->hyp_len, nbest->N, nbest->Th, nbest->max_len, nbest->coef, nbest->risk_scale, nbest->workspace};
    }
    if (kd) {
        if (!std::isfinite(kd->kd_scale)) { ishara_set_error("%s: kd_scale=%g is not finite", fn, (double)kd->kd_scale); return -1; }
        const int rc = kd_grad_check(fn, logits, kd->teacher, B, m->T, m->C, kd->inv_temp, kd->mode, nullptr, kd->kd_scale / (float)B, dl, 1, nullptr, kd->kl_frame, kd->kl_clip);
        if (rc != 0) return rc;
    }
    return keras_loss_backward(fn, m, logits, labels, B, loss, nll, loss_scale, frame_len, st, nbest ? &nb : nullptr, kd);
}
