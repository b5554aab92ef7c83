// The Keras get_model hybrid family, part 1: the layer graph get_model(...) builds (conv-hybrid-model.ipynb c7:12-65) with its gradient buckets,
// and the workspace plan (weight shadows first, then every activation and temporary of the forward / backward orchestration in
// conv_block.hip and keras_hybrid.hip).
#include "model_types.h"
#include <stdlib.h>

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
