// The Keras get_model hybrid family: the layer graph get_model(...) builds (conv-hybrid-model.ipynb c7:12-65), its workspace plan and
// the forward / backward orchestration over the kernels in gemm_nt.hip, gemm_tn.hip, norm_rows.hip, dwconv.hip, bn_gate.hip, attention.hip and ctc.hip.  confconv_fwd / _bwd
// also serve the torch families, ln_as_prologue and classifier_fwd the operator entry points (api_ops.hip).
#include "model_types.h"
#include <stdlib.h>

__global__ void droppath_kernel(float* rs, int B, DropSpec d) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) rs[b] = (d.thr == 0u || rng_keep(rng_row_key(d.key, (uint32_t)b), 0u, d.thr)) ? d.scale : 0.f;
}

// ------------------------------------------------------------------ construction
static void build_conv(ishara_model* m, const std::string& name, int k) {
    ConvBlock cb;
    const int d = m->d, c = 2 * d;
    cb.k = k;
    cb.W1 = m->dense(name + "_expand_conv", d, c, true);
    cb.dw = m->addp(name + "_dwconv/depthwise_kernel", k, c, true);
    cb.bn = m->bnp(name + "_bn", c);
    cb.eca = m->addp(name + "_eca/kernel", 5, 0, true);
    cb.W2 = m->dense(name + "_project_conv", c, d, true);
    cb.site = m->nsites++;
    m->convs.push_back(cb);
    m->layers.push_back({Layer::CONV, (int)m->convs.size() - 1});
    m->layer_entry_end.push_back(m->entries.size());
}
static FFN build_ffn(ishara_model* m, Norm ln, float eps, const std::string& n1, const std::string& n2, int e, bool out_drop) {
    FFN f; f.ln = ln; f.eps = eps;
    f.Wa = m->dense(n1, m->d, m->d * e, true);
    f.Wb = m->dense(n2, m->d * e, m->d, true);
    f.site_in = m->nsites++;
    f.has_out_drop = out_drop;
    if (out_drop) f.site_out = m->nsites++;
    return f;
}
static MHSA build_mhsa(ishara_model* m, Norm ln, float eps, const std::string& name, float rate, bool out_drop) {
    MHSA a; a.ln = ln; a.eps = eps; a.rate = rate;
    a.Wqkv = m->dense(name + "/qkv", m->d, 3 * m->d, false);
    a.Wp = m->dense(name + "/proj", m->d, m->d, false);
    a.site_attn = m->nsites++;
    a.has_out_drop = out_drop;
    if (out_drop) a.site_out = m->nsites++;
    return a;
}

void keras_build_graph(ishara_model* m) {
    const ishara_config& c = m->cfg;
    const int d = m->d;
    m->stemW = m->dense("stem_conv", m->F, d, false);
    m->stem_bn = m->bnp("stem_bn", d);
    m->stem_entry_end = m->entries.size();
    auto conv_blocks = [&](const std::string& tag) {
        for (int j = 0; j < c.num_conv_per_block; ++j) {
            const int k = c.kernel_sizes[j % c.num_kernel_sizes];
            build_conv(m, "conv" + tag + "_" + std::to_string(j + 1), k);
        }
    };
    const int esq = c.squeeze_expansion > 0 ? c.squeeze_expansion : c.expansion_factor;
    const int ecf = c.conformer_expansion > 0 ? c.conformer_expansion : c.expansion_factor;
    const int tk = c.transformer_kernel_size;
    for (int i = 0; i < c.num_conv_squeeze_blocks; ++i) {
        conv_blocks("squeeze_" + std::to_string(i));
        const std::string n = "squeezeformer_" + std::to_string(i);
        SqzBlock sb;
        // parameter order = oracle/ishara_oracle.py::_squeezeformer_specs
        Norm n1 = m->norm(n + "/norm1", d);
        sb.ffn1 = build_ffn(m, n1, 1e-6f, n + "/ffn1_dense1", n + "/ffn1_dense2", esq, true);
        Norm n2 = m->norm(n + "/norm2", d);
        sb.mha = build_mhsa(m, n2, 1e-6f, n + "/mha", c.dropout_rate, true);
        sb.conv.ln = m->norm(n + "/conv/norm", d);
        sb.conv.k = tk;
        sb.conv.Wc1 = m->dense(n + "/conv/conv1", d, d * esq, true);
        sb.conv.dw = m->addp(n + "/conv/conv2/depthwise_kernel", tk, d * esq, true);
        sb.conv.Wc3 = m->dense(n + "/conv/conv3", d * esq, d, true);
        sb.conv.R = d / 8 > 1 ? d / 8 : 1;
        sb.conv.seW1 = m->addp(n + "/conv/se/fc1/kernel", d, sb.conv.R, true);
        sb.conv.seb1 = m->addp(n + "/conv/se/fc1/bias", sb.conv.R, 0, true);
        sb.conv.seW2 = m->addp(n + "/conv/se/fc2/kernel", sb.conv.R, d, true);
        sb.conv.seb2 = m->addp(n + "/conv/se/fc2/bias", d, 0, true);
        Norm n3 = m->norm(n + "/norm3", d);
        sb.ffn2 = build_ffn(m, n3, 1e-6f, n + "/ffn2_dense1", n + "/ffn2_dense2", esq, true);
        m->sqz.push_back(sb);
        m->layers.push_back({Layer::SQZ, (int)m->sqz.size() - 1});
        m->layer_entry_end.push_back(m->entries.size());
    }
    for (int i = 0; i < c.num_conv_conform_blocks; ++i) {
        conv_blocks("conform_" + std::to_string(i));
        const std::string n = "conformer_" + std::to_string(i);
        ConfBlock cb;
        // order = _conformer_specs: ffn1, mha, conv (pw1, dw, pw2, bn, ln), ffn2, layer_norm1, layer_norm2
        Norm dummy;
        cb.ffn1 = build_ffn(m, dummy, 1e-6f, n + "/ffn1/dense1", n + "/ffn1/dense2", ecf, false);
        cb.mha = build_mhsa(m, dummy, 1e-6f, n + "/mha", c.conformer_attn_dropout, false);
        cb.conv.k = tk;
        cb.conv.Wp1 = m->dense(n + "/conv/pointwise_conv1", d, 2 * d, true);
        cb.conv.dw = m->addp(n + "/conv/depthwise_conv/kernel", tk, d, true);
        cb.conv.dwb = m->addp(n + "/conv/depthwise_conv/bias", d, 0, true);
        cb.conv.Wp2 = m->dense(n + "/conv/pointwise_conv2", d, d, true);
        cb.conv.bn = m->bnp(n + "/conv/batch_norm", d);
        cb.conv.ln = m->norm(n + "/conv/layer_norm", d);
        cb.ffn2 = build_ffn(m, dummy, 1e-6f, n + "/ffn2/dense1", n + "/ffn2/dense2", ecf, false);
        Norm l1 = m->norm(n + "/layer_norm1", d);
        Norm l2 = m->norm(n + "/layer_norm2", d);
        cb.ffn1.ln = l1; cb.mha.ln = l1;      // layer_norm1 is applied twice (c5:324,330)
        cb.ffn2.ln = l2;
        // dropout sites were numbered in build order ffn1, mha, ffn2 == forward order
        m->conf.push_back(cb);
        m->layers.push_back({Layer::CONF, (int)m->conf.size() - 1});
        m->layer_entry_end.push_back(m->entries.size());
    }
    m->topW = m->dense("top_conv", d, m->dtop, true);
    m->clsW = m->dense("classifier", m->dtop, m->C, true);
    m->head_site = m->nsites++;

    finish_param_layout(m);

    // ---- gradient buckets.  Trainable parameters sit in creation order (stem, layers, head) and the backward pass runs head ->
    // layers in reverse -> stem, so the gradient of everything above a layer boundary is final once that layer's backward is
    // enqueued: up to 4 ranges of about equal size, cut at layer boundaries, each with an event recorded on the compute stream.
    {
        const int nl = (int)m->layers.size();
        auto first_off = [&](size_t e0) -> int64_t {           // offset of the first trainable entry at index >= e0
            for (size_t i = e0; i < m->entries.size(); ++i) if (m->entries[i].trainable) return m->entries[i].offset;
            return m->n_train;
        };
        std::vector<int64_t> lo(nl);                            // first gradient element of layer li
        for (int li = 0; li < nl; ++li) lo[li] = first_off(li == 0 ? m->stem_entry_end : m->layer_entry_end[li - 1]);
        const int64_t target = m->n_train / 4 + 1;
        int64_t hi = m->n_train;
        m->bucket_after_layer.assign(nl, -1);
        for (int li = nl - 1; li >= 1 && (int)m->bucket_lo.size() < 3; --li) {
            if (hi - lo[li] >= target && lo[li] > 0) {          // cut below layer li: bucket = [lo[li], hi)
                m->bucket_after_layer[li] = (int)m->bucket_lo.size();
                m->bucket_lo.push_back(lo[li]); m->bucket_hi.push_back(hi);
                hi = lo[li];
            }
        }
        m->bucket_lo.push_back(0); m->bucket_hi.push_back(hi);  // the rest (stem included): complete at the end of the backward pass
    }
}

void keras_plan_workspace(ishara_model* m) {
    const int d = m->d, B = m->Bmax, T = m->T;
    const size_t Mx = (size_t)B * T;
    m->cur = 0;
    // ---- shadows first (one contiguous arena that sync_weights zero-fills)
    m->shadow_begin = m->cur;
    m->stem_kp = (dt_is16(m->dt) && m->F <= 512) ? (m->F <= 256 ? 256 : 512) : 0;      // fp16 (inference) too: the stem Dense on the A-stationary kernel
    plan_shadow(m, m->stemW, m->stem_kp);
    for (auto& cb : m->convs) { plan_shadow(m, cb.W1); plan_shadow(m, cb.W2); }
    // FFN/MHSA shadows are planned with their activations below; keep the arena contiguous by
    // planning all shadows before any activation:
    std::vector<DenseW*> later;
    for (auto& sb : m->sqz) { later.insert(later.end(), {&sb.ffn1.Wa, &sb.ffn1.Wb, &sb.mha.Wqkv, &sb.mha.Wp, &sb.conv.Wc1, &sb.conv.Wc3, &sb.ffn2.Wa, &sb.ffn2.Wb}); }
    for (auto& cb : m->conf) { later.insert(later.end(), {&cb.ffn1.Wa, &cb.ffn1.Wb, &cb.mha.Wqkv, &cb.mha.Wp, &cb.conv.Wp1, &cb.conv.Wp2, &cb.ffn2.Wa, &cb.ffn2.Wb}); }
    later.push_back(&m->topW); later.push_back(&m->clsW);
    // classifier: its dY operand is the zero-padded bf16 [M, 128] copy of dlogits (bf16 model, <= 64 classes)
    m->cls_pad = (m->dt == DT_BF16 && m->C <= 64 && m->C % 4 == 0) ? 128 : 0;
    for (DenseW* w : later) plan_shadow(m, *w, 0, w == &m->clsW ? m->cls_pad : 0);
    m->shadow_end = m->cur;
    m->shadow_tab_off = m->alloc(m->denses.size() * sizeof(ShadowDesc)).off;
    // ---- stem
    m->pe = m->f32((size_t)T * d);
    m->stem_h0 = m->act(d); m->stem_out = m->act(d);
    if (m->stem_kp) m->stem_xb = m->alloc(Mx * (size_t)m->stem_kp * 2);
    m->stem_ssum = m->f32((size_t)B * d); m->stem_ssq = m->f32((size_t)B * d);
    m->stem_mean = m->f32(d); m->stem_rstd = m->f32(d); m->stem_a = m->f32(d); m->stem_bsh = m->f32(d);
    for (auto& cb : m->convs) {
        const int c = 2 * d;
        cb.z1 = m->act(c); cb.h2 = m->act(c); cb.h4 = m->act(c); cb.out = m->act(d);
        cb.ssum = m->f32((size_t)B * c); cb.ssq = m->f32((size_t)B * c);
        cb.mean = m->f32(c); cb.rstd = m->f32(c); cb.a = m->f32(c); cb.bsh = m->f32(c);
        cb.gn = m->f32((size_t)B * c); cb.sg = m->f32((size_t)B * c); cb.P = m->f32((size_t)B * c); cb.Q = m->f32((size_t)B * c);
        cb.rs = m->f32(B);
    }
    auto plan_ffn_act = [&](FFN& f) {
        f.xn = m->act(d); f.mean = m->f32(Mx); f.rstd = m->f32(Mx);
        f.za = m->act(f.Wa.N); f.u = m->act(f.Wa.N); f.out = m->act(d);
    };
    auto plan_mhsa_act = [&](MHSA& a) {
        a.xn = m->act(d); a.mean = m->f32(Mx); a.rstd = m->f32(Mx);
        a.q = m->act(d); a.k = m->act(d); a.vt = m->act(d); a.o = m->act(d);
        a.lse = m->f32((size_t)B * m->H * T); a.out = m->act(d);
        a.maskw = m->f32(attn_mask_words(B, m->H, T));        // dropout keep bits of the attention probabilities (fwd -> bwd)
    };
    for (auto& sb : m->sqz) {
        plan_ffn_act(sb.ffn1); plan_mhsa_act(sb.mha);
        SqzConv& c = sb.conv;
        const int de = c.Wc1.N;
        c.xn = m->act(d); c.mean = m->f32(Mx); c.rstd = m->f32(Mx);
        c.zc = m->act(de); c.zd = m->act(de); c.hd = m->act(de); c.u3 = m->act(d);
        c.gap = m->f32((size_t)B * d); c.hid = m->f32((size_t)B * c.R); c.se = m->f32((size_t)B * d); c.out = m->act(d);
        plan_ffn_act(sb.ffn2);
    }
    for (auto& cb : m->conf) {
        plan_ffn_act(cb.ffn1); plan_mhsa_act(cb.mha);
        plan_confconv(m, cb.conv, Mx, B, d);
        plan_ffn_act(cb.ffn2);
    }
    m->head_hh = m->act(m->dtop);
    // ---- temporaries
    int maxw = 3 * d;
    if (m->dtop > maxw) maxw = m->dtop;
    for (auto& sb : m->sqz) if (sb.ffn1.Wa.N > maxw) maxw = sb.ffn1.Wa.N;
    for (auto& cb : m->conf) if (cb.ffn1.Wa.N > maxw) maxw = cb.ffn1.Wa.N;
    m->gA = m->act(d); m->gB = m->act(d);
    m->t1 = m->act(maxw); m->t2 = m->act(maxw); m->t3 = m->act(maxw);
    const int maxc = 2 * d > maxw ? 2 * d : maxw;
    m->S1 = m->f32((size_t)B * maxc); m->S2 = m->f32((size_t)B * maxc); m->E = m->f32((size_t)B * maxc);
    m->Fc = m->f32(maxc); m->Ecol = m->f32(maxc); m->ecap = m->f32((size_t)B * 8 * ECA_MAX_CHUNKS);
    m->dse = m->f32((size_t)B * d); m->dgapT = m->f32((size_t)B * d);
    m->psa_on = m->dt == DT_BF16 && !m->convs.empty() && getenv("ISHARA_NO_PSA") == nullptr;
    if (m->psa_on) { m->psaG = m->f32((size_t)B * d); m->psaR = m->f32((size_t)B * (size_t)((d + 63) / 64) * 2 * d); }
    m->slab = m->f32(slab_floats(m, Mx, B, T, maxw));
    { const size_t wf = wgrad_slab_floats(m, Mx);
      m->slab2[0] = m->f32(wf); m->slab2[1] = m->f32(wf); m->tn_defer_on = getenv("ISHARA_NO_DEFERRED_SLAB_SUMS") == nullptr; }
    {   // arena of the deferred parameter-gradient sums: every LayerNorm / depthwise-conv backward of one pass (flushed early when it runs full)
        size_t need = 0;
        const size_t lnf = (layernorm_bwd_scratch_floats(d) + 63) & ~(size_t)63, dwf = (dwconv_bwd_scratch_floats(2 * maxw, 31) + 63) & ~(size_t)63;
        need = (size_t)m->layers.size() * (5 * lnf + 2 * dwf);
        const size_t cap = (size_t)256 << 20;                       // floats: 1 GiB
        m->red_cap = need < cap ? need : cap;
        m->red_on = getenv("ISHARA_NO_DEFERRED_REDUCE") == nullptr && m->red_cap > 0;
        if (m->red_on) m->red_arena = m->f32(m->red_cap);
    }
    m->ctcws = m->f32(ctc_workspace_floats(B, T, m->L));
    m->dlogits = m->f32(Mx * m->C);
    if (m->cls_pad) m->dlb = m->alloc(Mx * (size_t)m->cls_pad * 2);
    m->nllb = m->f32(B);
    m->delta = m->f32((size_t)B * m->H * T);
    m->ws_need = m->cur;
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
static int conv_fwd(ishara_model* m, ConvBlock& cb, const Run& r, const void* x) {
    const int d = m->d, c = 2 * d, B = r.B, T = m->T, dt = m->dt;
    OpArgs no; EpiArgs e1;
    CK(gemm_fwd(m, cb.W1, x, dt, m->W(cb.z1), dt, r.M, OP_NONE, no, e1));
    // inference: the partial statistic rows of the depthwise conv are summed, and the BatchNorm constants formed from the moving statistics,
    // inside eca_fwd (4 launches per Conv1DBlock instead of 6: at B = 1 every launch is ~9 us of latency)
    // Frame lengths (r.key_len; DESIGN §2 "Frame lengths"): the ECA gate pools BN(h2) over the clip's n_b valid frames (c5:8-9).  BatchNorm's statistics
    // stay over all B*T rows, so the depthwise conv's statistics pass runs as without lengths; a masked time mean of h2 (a kernel of its own) then
    // feeds eca_fwd_len (g = 0 at n_b = 0).  The fused inference form and the psa weight gradient assume the all-T sums: not taken.
    const int* fl = r.key_len;
    int prows = 0;
    const bool infer_fused = !r.training && !fl && getenv("ISHARA_NO_INFER_FUSION") == nullptr;
    static const bool no_train_fusion = getenv("ISHARA_NO_STATS_FUSION") != nullptr;
    const bool train_fused = r.training && !no_train_fusion;
    CKP(m, "dwconv_fwd", 3.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_dwconv_fwd(dt, DWIN_SWISH, m->W(cb.z1), m->P(cb.dw), nullptr, m->W(cb.h2), m->Wf(cb.ssum), m->Wf(cb.ssq), m->Wf(m->slab), B, T, c, cb.k, cb.k - 1, m->s,
                                                                                          (infer_fused || train_fused) ? &prows : nullptr));
    if (train_fused && prows > 0)      // training: batch statistics straight from the partial rows [B * prows][2][C] (no stats_reduce launch; eca_fwd below sums them per sample)
    CKP(m, "bn_finalize", 0, 0, launch_bn_finalize(m->Wf(m->slab), m->Wf(m->slab) + c, B * prows, (float)B * T, m->P(cb.bn.gamma), m->P(cb.bn.beta), 1e-3f, 0.95f,
                          m->P(cb.bn.mm), m->P(cb.bn.mv), r.training, m->Wf(cb.mean), m->Wf(cb.rstd), m->Wf(cb.a), m->Wf(cb.bsh), c, m->s, 1.f, 2 * c));
    else if (!(infer_fused && prows > 0))
    CKP(m, "bn_finalize", 0, 0, launch_bn_finalize(m->Wf(cb.ssum), m->Wf(cb.ssq), B, (float)B * T, m->P(cb.bn.gamma), m->P(cb.bn.beta), 1e-3f, 0.95f,
                          m->P(cb.bn.mm), m->P(cb.bn.mv), r.training, m->Wf(cb.mean), m->Wf(cb.rstd), m->Wf(cb.a), m->Wf(cb.bsh), c, m->s));
    // Drop-path (c5:82-83) on the branch: y = x + rs[b] * (h4 W2 + b2).  Where the fast kernels apply, rs[b] is folded into the per-sample
    // affine that produces h4 (h4 = rs[b] * (h2 P + Q), free), the GEMM adds rs[b] * b2, and the backward pass needs no scaled copy of
    // the incoming gradient: dgrad scales its OUTPUT rows, wgrad multiplies h4^T by the plain gradient and weights the bias sum.
    const DropSpec ds = dspec(r, cb.site, m->cfg.dropout_rate);
    EpiArgs e2; e2.resid = x;
    cb.folded = false; cb.psa = false;
    if (ds.thr) {                                        // rs[b] itself is drawn by eca_fwd below (one launch less per block)
        e2.rowscale = m->Wf(cb.rs); e2.T = T;
        EpiArgs probe = e2; probe.bias = m->P(cb.W2.b);
        cb.folded = dt == DT_BF16 && !g_force_regstage && gemm_nt_as_applicable(dt, r.M, cb.W2.N, cb.W2.K, cb.W2.ldt, probe) && gemm_nt_as_applicable(dt, r.M, cb.W2.K, cb.W2.N, cb.W2.ldn, probe) &&
                    gemm_tn_bias_rowscale_ok(dt, dt, dt, r.M, cb.W2.K, cb.W2.N, T);
        e2.rowscale_bias = cb.folded ? 1 : 0;
    }
    if (fl) {
        CKP(m, "masked_time_mean", 1.0 * r.M * c * (double)dt_size(dt), 0, launch_masked_time_mean(dt, m->W(cb.h2), fl, m->Wf(cb.ssum), B, T, c, m->s));
        CKP(m, "eca_fwd_len", 0, 0, launch_eca_fwd_len(m->Wf(cb.ssum), m->Wf(cb.a), m->Wf(cb.bsh), m->P(cb.eca), fl, T, m->Wf(cb.gn), m->Wf(cb.sg), m->Wf(cb.P), m->Wf(cb.Q), B, c, m->s, ds.thr ? m->Wf(cb.rs) : nullptr, ds, cb.folded ? 1 : 0));
    } else if (infer_fused && prows > 0)
        CKP(m, "eca_fwd", 0, 0, launch_eca_fwd_infer(m->Wf(m->slab), prows, m->P(cb.bn.mm), m->P(cb.bn.mv), m->P(cb.bn.gamma), m->P(cb.bn.beta), 1e-3f, m->P(cb.eca), 1.f / T,
                                                       m->Wf(cb.gn), m->Wf(cb.sg), m->Wf(cb.P), m->Wf(cb.Q), B, c, m->s));
    else if (train_fused && prows > 0)
        CKP(m, "eca_fwd", 0, 0, launch_eca_fwd_part(m->Wf(m->slab), prows, m->Wf(cb.ssum), m->Wf(cb.a), m->Wf(cb.bsh), m->P(cb.eca), 1.f / T, m->Wf(cb.gn), m->Wf(cb.sg), m->Wf(cb.P), m->Wf(cb.Q), B, c, m->s,
                                                      ds.thr ? m->Wf(cb.rs) : nullptr, ds, cb.folded ? 1 : 0));
    else
    CKP(m, "eca_fwd", 0, 0, launch_eca_fwd(m->Wf(cb.ssum), m->Wf(cb.a), m->Wf(cb.bsh), m->P(cb.eca), 1.f / T, m->Wf(cb.gn), m->Wf(cb.sg), m->Wf(cb.P), m->Wf(cb.Q), B, c, m->s, ds.thr ? m->Wf(cb.rs) : nullptr, ds, cb.folded ? 1 : 0));
    // h4 = h2 * P[b] + Q[b] (BatchNorm + ECA gate [+ drop-path]) as a prologue of the project GEMM: h2 is read once, h4 is written from
    // the transformed fragments for the weight-gradient GEMM (training only); other shapes run the separate affine pass
    {
        EpiArgs probe = e2; probe.pa_P = m->Wf(cb.P); probe.pa_Q = m->Wf(cb.Q); probe.T = T; probe.bias = m->P(cb.W2.b);
        probe.pro_out = r.training ? m->W(cb.h4) : nullptr;
        if (gemm_nt_as_prologue_ok(dt, dt, dt, r.M, cb.W2.N, cb.W2.K, cb.W2.ldt, probe)) {
            // training: h4 is written only when the backward pass needs it in memory — not when the project conv's weight-gradient GEMM applies
            // P, Q itself (gemm_tn.hip TnPsa: whole samples per M-split; the drop-path scale, if any, must be the folded one)
            cb.psa = r.training && m->psa_on && !fl && (!ds.thr || cb.folded) && gemm_tn_psa_ok(dt, dt, dt, r.M, cb.W2.K, cb.W2.N, T);
            e2.pa_P = m->Wf(cb.P); e2.pa_Q = m->Wf(cb.Q); e2.T = T; e2.pro_out = (r.training && !cb.psa) ? m->W(cb.h4) : nullptr;
            CK(gemm_fwd(m, cb.W2, m->W(cb.h2), dt, m->W(cb.out), dt, r.M, OP_NONE, no, e2));
            return 0;
        }
    }
    CKP(m, "sample_affine", 4.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_affine(dt, m->W(cb.h2), m->Wf(cb.P), m->Wf(cb.Q), nullptr, m->W(cb.h4), B, T, c, m->s));
    CK(gemm_fwd(m, cb.W2, m->W(cb.h4), dt, m->W(cb.out), dt, r.M, OP_NONE, no, e2));
    return 0;
}

static int ffn_fwd(ishara_model* m, FFN& f, const Run& r, const void* x) {
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

static int mhsa_fwd(ishara_model* m, MHSA& a, const Run& r, const void* x) {
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

static int sqzconv_fwd(ishara_model* m, SqzConv& c, const Run& r, const void* x) {
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
    int prows = 0;
    static const bool no_train_fusion = getenv("ISHARA_NO_STATS_FUSION") != nullptr;
    const bool train_fused = r.training && !no_train_fusion;        // batch statistics straight from the depthwise conv's partial rows: no stats_reduce launch
    CKP(m, "dwconv_fwd", 3.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_dwconv_fwd(dt, DWIN_GLU, m->W(c.g), m->P(c.dw), c.dwb >= 0 ? m->P(c.dwb) : nullptr, m->W(c.v), r.training ? m->Wf(c.ssum) : nullptr, r.training ? m->Wf(c.ssq) : nullptr, m->Wf(m->slab), B, T, d, c.k, (c.k - 1) / 2, m->s,
                                                                                          train_fused ? &prows : nullptr));      // inference: no batch statistics
    const float var_corr = c.bn_unbiased && B * T > 1 ? (float)((double)B * T / ((double)B * T - 1.0)) : 1.f;
    if (train_fused && prows > 0)
    CKP(m, "bn_finalize", 0, 0, launch_bn_finalize(m->Wf(m->slab), m->Wf(m->slab) + d, B * prows, (float)B * T, m->P(c.bn.gamma), m->P(c.bn.beta), c.bn_eps, c.bn_keep,
                          m->P(c.bn.mm), m->P(c.bn.mv), r.training, m->Wf(c.mean), m->Wf(c.rstd), m->Wf(c.a), m->Wf(c.bsh), d, m->s, var_corr, 2 * d));
    else
    CKP(m, "bn_finalize", 0, 0, launch_bn_finalize(m->Wf(c.ssum), m->Wf(c.ssq), B, (float)B * T, m->P(c.bn.gamma), m->P(c.bn.beta), c.bn_eps, c.bn_keep,
                          m->P(c.bn.mm), m->P(c.bn.mv), r.training, m->Wf(c.mean), m->Wf(c.rstd), m->Wf(c.a), m->Wf(c.bsh), d, m->s, var_corr));
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
    const bool fusion = getenv("ISHARA_NO_INFER_FUSION") == nullptr;
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
static int stem_fwd(ishara_model* m, const Run& r, const float* x) {
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
static int head_fwd(ishara_model* m, const Run& r, const void* h, float* logits) {
    const int dt = m->dt;
    OpArgs no;
    // ---- head: Dense(relu) -> Dropout(0.4) -> Dense  (c7:61-63)
    EpiArgs et; et.act = ACT_RELU; et.drop = dspec(r, m->head_site, m->cfg.head_dropout);
    CK(gemm_fwd(m, m->topW, h, dt, m->W(m->head_hh), dt, r.M, OP_NONE, no, et));
    CK(classifier_fwd(m, CLS_AUTO, dt, m->W(m->head_hh), m->ws + m->clsW.wt, m->clsW.ldt, m->clsW.b >= 0 ? m->P(m->clsW.b) : nullptr, logits, r.M, m->clsW.K, m->C, m->s));
    return 0;
}

// what every entry point that takes frame lengths refuses before any GPU work (frame_len == NULL: nothing to refuse)
static bool frame_len_ok(const ishara_model* m, const char* fn, const int32_t* frame_len) {
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

// ------------------------------------------------------------------ module backward
static const void* layer_out(ishara_model* m, const Layer& L) {      // output activation of a layer of the sequential graph
    return L.kind == Layer::CONV ? m->W(m->convs[L.idx].out) : (L.kind == Layer::SQZ ? m->W(m->sqz[L.idx].ffn2.out) : m->W(m->conf[L.idx].ffn2.out));
}
// each *_bwd consumes g (grad wrt the module output) and writes gn (grad wrt its input x)
static int conv_bwd(ishara_model* m, ConvBlock& cb, const Run& r, const void* x, const void* g, void* gn) {
    const int d = m->d, c = 2 * d, B = r.B, T = m->T, dt = m->dt;
    OpArgs no;
    const DropSpec ds = dspec(r, cb.site, m->cfg.dropout_rate);
    const void* gs = g;                                  // gradient through the drop-path: dY * rs[b]
    EpiArgs e1;
    if (cb.psa) {                                        // h4 was never written: dW2 = sum_b diag(P_b) h2_b^T g_b + Q_b x colsum(g_b) inside the GEMM, which
        const float* rs = ds.thr ? m->Wf(cb.rs) : nullptr;   // also emits the statistics of dh4 (S1, S2 below) — no pass over dh4 and h2
        if (rs) { e1.rowscale = rs; e1.T = T; }
        CK(gemm_dgrad(m, cb.W2, g, dt, m->W(m->t1), r.M, OP_NONE, no, e1));
        TnPsa ps; ps.P = m->Wf(cb.P); ps.Q = m->Wf(cb.Q); ps.W = m->ws + cb.W2.wn; ps.ldw = cb.W2.ldn; ps.G = m->Wf(m->psaG); ps.Rpart = m->Wf(m->psaR); ps.T = T;
        { static const int psa_dbg = getenv("ISHARA_PSA_DBG") ? atoi(getenv("ISHARA_PSA_DBG")) : 0; ps.dbg = psa_dbg; }
        CK(gemm_wgrad(m, cb.W2, m->W(cb.h2), dt, OP_NONE, no, g, dt, OP_NONE, no, r.M, 0, 0, rs, rs ? T : 0, &ps));
    } else if (ds.thr && cb.folded) {                    // h4 carries rs[b] (conv_fwd): dh4 = (g W2^T) * rs[b]; dW2 = h4^T g; db2 = sum_m rs[b(m)] g[m]
        e1.rowscale = m->Wf(cb.rs); e1.T = T;
        CK(gemm_dgrad(m, cb.W2, g, dt, m->W(m->t1), r.M, OP_NONE, no, e1));
        CK(gemm_wgrad(m, cb.W2, m->W(cb.h4), dt, OP_NONE, no, g, dt, OP_NONE, no, r.M, 0, 0, m->Wf(cb.rs), T));
    } else {
        if (ds.thr) {
            CKP(m, "map_rows", 2.0 * r.M * d * (double)dt_size(m->dt), 0, launch_map_rows(dt, MAP_ROWSCALE, g, m->W(m->t3), m->Wf(cb.rs), ds, r.M, T, d, m->s));
            gs = m->W(m->t3);
        }
        CK(gemm_dgrad(m, cb.W2, gs, dt, m->W(m->t1), r.M, OP_NONE, no, e1));                       // dh4
        CK(gemm_wgrad(m, cb.W2, m->W(cb.h4), dt, OP_NONE, no, gs, dt, OP_NONE, no, r.M));
    }
    if (!cb.psa) CKP(m, "sample_reduce", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_reduce(dt, m->W(m->t1), m->W(cb.h2), m->Wf(cb.mean), m->Wf(cb.rstd), m->Wf(m->S1), m->Wf(m->S2), B, T, c, m->s));
    PsaStats pst;                                        // cb.psa: S1, S2 come out of the finalize kernel itself (from G and Rpart)
    if (cb.psa) { pst.G = m->Wf(m->psaG); pst.Rpart = m->Wf(m->psaR); pst.nparts = cb.W2.N / 64; pst.Wt = m->ws + cb.W2.wt; pst.ldt = cb.W2.ldt; pst.N = cb.W2.N;
                  pst.rs = ds.thr ? m->Wf(cb.rs) : nullptr; pst.mean = m->Wf(cb.mean); pst.rstd = m->Wf(cb.rstd); }
    CKP(m, "eca_bn_bwd_finalize", 0, 0, launch_eca_bn_bwd_finalize(m->Wf(m->S1), m->Wf(m->S2), m->Wf(cb.ssum), m->Wf(cb.gn), m->Wf(cb.sg), m->P(cb.eca), m->P(cb.bn.gamma), m->P(cb.bn.beta),
                                  m->Wf(cb.mean), m->Wf(cb.rstd), m->G(cb.bn.gamma), m->G(cb.bn.beta), m->G(cb.eca), m->Wf(m->E), m->Wf(m->Fc), m->Wf(m->ecap), B, T, c, m->s, cb.psa ? &pst : nullptr, r.key_len, m->Wf(m->Ecol)));
    if (r.key_len) {      // frame lengths: the gate's gradient E[b,c] = dgn / n_b reaches the frames t < n_b only, Ecol[c] = -dbeta / Mtot every frame.  The two-kernel
        // path: the BatchNorm-carrying depthwise backward takes one constant per (sample, channel) (DESIGN §2 "Frame lengths": routes)
        CKP(m, "bn_bwd_apply_len", 6.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_bn_bwd_apply_len(dt, m->W(m->t1), m->W(cb.h2), m->Wf(cb.mean), m->Wf(cb.rstd), m->Wf(cb.a), m->Wf(cb.sg), m->Wf(m->E), m->Wf(m->Ecol), m->Wf(m->Fc), r.key_len, m->W(m->t1), B, T, c, m->s));
        CK(dwconv_bwd_deferred(m, r, 8.0, DWIN_SWISH, m->W(m->t1), nullptr, m->W(cb.z1), cb.dw, -1, m->W(m->t2), c, cb.k, cb.k - 1));
    } else {
    // BatchNorm backward applied inside the depthwise-conv backward (one pass over dh4, h2 and z1); shapes without the fused kernel
    // take the two-kernel path
    DwBnArgs bn; bn.h = m->W(cb.h2); bn.mean = m->Wf(cb.mean); bn.rstd = m->Wf(cb.rstd); bn.a = m->Wf(cb.a); bn.sg = m->Wf(cb.sg); bn.E = m->Wf(m->E); bn.Fc = m->Wf(m->Fc); bn.e_per_sample = 1;
    const int fused = dwconv_bwd_deferred(m, r, 10.0, DWIN_SWISH, m->W(m->t1), &bn, m->W(cb.z1), cb.dw, -1, m->W(m->t2), c, cb.k, cb.k - 1);
    if (fused < 0) return fused;
    if (!fused) {
        CKP(m, "bn_bwd_apply", 6.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_bn_bwd_apply(dt, m->W(m->t1), m->W(cb.h2), m->Wf(cb.mean), m->Wf(cb.rstd), m->Wf(cb.a), m->Wf(cb.sg), m->Wf(m->E), 1, m->Wf(m->Fc), m->W(m->t1), B, T, c, m->s));
        CK(dwconv_bwd_deferred(m, r, 8.0, DWIN_SWISH, m->W(m->t1), nullptr, m->W(cb.z1), cb.dw, -1, m->W(m->t2), c, cb.k, cb.k - 1));
    }
    }
    EpiArgs e2; e2.resid = g;
    CK(gemm_dgrad(m, cb.W1, m->W(m->t2), dt, gn, r.M, OP_NONE, no, e2));
    CK(gemm_wgrad(m, cb.W1, x, dt, OP_NONE, no, m->W(m->t2), dt, OP_NONE, no, r.M));
    return 0;
}

static int ffn_bwd(ishara_model* m, FFN& f, const Run& r, const void* x, const void* g, void* gn) {
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

static int mhsa_bwd(ishara_model* m, MHSA& a, const Run& r, const void* x, const void* g, void* gn) {
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

static int sqzconv_bwd(ishara_model* m, SqzConv& c, const Run& r, const void* x, const void* g, void* gn) {
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
    const int fused = dwconv_bwd_deferred(m, r, 6.0, DWIN_GLU, m->W(m->t2), &bn, m->W(c.g), c.dw, c.dwb, m->W(m->t3), d, c.k, (c.k - 1) / 2);   // dg [M,2d]
    if (fused < 0) return fused;
    if (!fused) {
        CKP(m, "bn_bwd_apply", 6.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_bn_bwd_apply(dt, m->W(m->t2), m->W(c.v), m->Wf(c.mean), m->Wf(c.rstd), m->Wf(c.a), nullptr, m->Wf(m->Ecol), 0, m->Wf(m->Fc), m->W(m->t2), B, T, d, m->s));   // dv
        CK(dwconv_bwd_deferred(m, r, 8.0, DWIN_GLU, m->W(m->t2), nullptr, m->W(c.g), c.dw, c.dwb, m->W(m->t3), d, c.k, (c.k - 1) / 2));   // dg [M,2d]
    }
    EpiArgs e2; e2.resid = m->W(m->t1);
    CK(gemm_dgrad(m, c.Wp1, m->W(m->t3), dt, gn, r.M, OP_NONE, no, e2));
    CK(gemm_wgrad(m, c.Wp1, x, dt, OP_NONE, no, m->W(m->t3), dt, OP_NONE, no, r.M));
    return 0;
}

// head backward: g = gradient with respect to the head's input hin, from dlogits / dlb (the CTC kernel wrote them)
static int head_bwd(ishara_model* m, const Run& r, const void* hin, void* g) {
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
static int stem_bwd(ishara_model* m, const Run& r, const void* g) {
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
static bool frame_len_agrees(const char* fn, bool fwd_had, const int32_t* frame_len) {
    if (fwd_had == (frame_len != nullptr)) return true;
    ishara_set_error("%s: the training forward was %s frame lengths, this call is %s", fn, fwd_had ? "given" : "not given", frame_len ? "given some" : "given none");
    return false;
}
static int keras_loss_backward(const char* fn, ishara_model* m, const float* logits, const int64_t* labels, int32_t B, float* loss, float* nll, float loss_scale, const int32_t* frame_len, ishara_stream st) {
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
