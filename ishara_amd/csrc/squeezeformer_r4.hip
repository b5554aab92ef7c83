// The torch Squeezeformer family of the reference (squeezeformer/{attention,modules,convolution,encoder}.py):
//   R1  RelativeMultiHeadAttention (attention.py:25-110): Transformer-XL attention — content score (q + u_bias) . k plus positional score
//       (q + v_bias) . p with p = pos_proj(RelPositionalEncoding); `_relative_shift` (:102-110) in closed form: the key j of query i
//       reads row T-1-i+j of the [2T-1, d] table.  Flash-style kernels (relattn_len.hip, relattn_mfma.hip; no [T, T] matrix in memory),
//       forward and three backward passes (dq + du/dv, dk/dv, dpos) that recompute the probabilities from the saved log-sum-exp.
//   R2  RelPositionalEncoding (modules.py:59-108): table built on the host at create time (fp32 sin / cos, positions T-1 .. -(T-1)).
//   R3  ConvModule (convolution.py:199-238): the ConfConv composition of keras_hybrid.hip with Swish after the BatchNorm, no depthwise bias.
//   R4  post-LN SqueezeformerBlock (encoder.py:208-247) with the half-step FFN residual, DepthwiseConv2dSubsampling
//       (convolution.py:39-73), TimeReductionLayer (:241-269), recover_resolution (modules.py:137-142) and the encoder loop
//       (encoder.py:135-166) with its ResidualConnectionModule around the reduced-rate blocks (:88-103).
// Parameter entries carry the reference's state_dict keys, in state_dict order, arrays in the kernels' layout (Linear / pointwise
// weights [in,out], 3x3 kernels [C,9], depthwise [k,d], u/v bias [d]); ishara_amd/squeezeformer.py converts to and from torch's.
// This file is the encoder itself: state, graph, workspace plan, bind, forward, backward and the entry points with per-clip lengths.  Its own
// kernels are in r4_subsample.hip (subsampling, time reduction, row maps, stage lengths) and relattn_len.hip / relattn_mfma.hip (attention).
#include "model_types.h"

static const float R4_EPS = 1e-5f;

// ------------------------------------------------------------------ state
struct RelMHSA {
    DenseW Wq, Wk, Wv, Wpos, Wo; int u = -1, v = -1; Norm ln; uint32_t site_attn = 0, site_out = 0;
    Buf q, k, vv, o, lse, posp, r, mean, rstd, out;
};
struct R4Layer { RelMHSA mha; R5FFN ffn1; ConfConv conv; R5FFN ffn2; int T = 0; bool wrapped = false; Buf wrap_out; int pe = 0; int stage = 0; };      // stage: 0 at T2, 1 reduced (T3), 2 recovered (Trec)
struct R4State {
    int w1 = -1, b1 = -1, w2 = -1, b2 = -1, trw = -1, trb = -1;
    DenseW Win, Wred, Wrec;
    int T0 = 0, F = 0, T1 = 0, F1 = 0, T2 = 0, F2 = 0, T3 = 0, Fr = 0, Kp = 0, Trec = 0, Tout = 0;
    int reduce = 0, recover = 0; uint32_t site_in = 0;
    Buf y1, dz1, dwred, sub, h0, trpre, trout, red, rep, crop, rec, gskip, gwrap, dsub, dqb, dkb, dvb, dposp;
    Buf nlen;      // int32 [3][Bmax]: keys per clip at T2 / T3 / Trec, derived from the caller's input lengths by the masked pass (r4_stage_len_launch)
    std::vector<R4Layer> layers;
    std::vector<int> pe_T; std::vector<Buf> pe32, pedt; std::vector<std::vector<float>> pe_host;
};

// ------------------------------------------------------------------ construction
static R5FFN r4_build_ffn(ishara_model* m, const std::string& mod, const std::string& ln, float factor) {
    R5FFN f;
    const int d = m->d, e = m->cfg.expansion_factor;
    f.W1 = m->dense_named(mod + ".sequential.0.weight", mod + ".sequential.0.bias", d, d * e);
    f.W2 = m->dense_named(mod + ".sequential.3.weight", mod + ".sequential.3.bias", d * e, d);
    f.ln = m->norm_named(ln, d);
    f.site_in = m->nsites++; f.site_out = m->nsites++;
    f.factor = factor;
    return f;
}

int r4_validate(const ishara_config& c) {
    if (c.num_conv_conform_blocks <= 0) { ishara_set_error("SqueezeformerEncoder: num_layers (num_conv_conform_blocks) must be > 0"); return -1; }
    if (c.features < 7) { ishara_set_error("SqueezeformerEncoder: input_dim (features) must be >= 7 (two 3x3 stride-2 convolutions)"); return -1; }
    if (c.frames < 7) { ishara_set_error("SqueezeformerEncoder: frames must be >= 7"); return -1; }
    const int dh = c.dim / c.num_heads;
    if (!relattn_head_dim_ok(dh)) { ishara_set_error("SqueezeformerEncoder: head dim %d unsupported (" RELATTN_HEAD_DIMS ")", dh); return -1; }
    const int L = c.num_conv_conform_blocks;
    if (c.reduce_layer_index < L && c.recover_layer_index < L && c.recover_layer_index <= c.reduce_layer_index) { ishara_set_error("SqueezeformerEncoder: recover_layer_index must follow reduce_layer_index"); return -1; }
    if (c.reduce_layer_index >= L && c.recover_layer_index < L) { ishara_set_error("SqueezeformerEncoder: recover without reduce"); return -1; }
    if (c.reduce_layer_index < 0 || c.recover_layer_index < 0) { ishara_set_error("SqueezeformerEncoder: negative layer index"); return -1; }
    return 0;
}

void r4_build_graph(ishara_model* m) {
    R4State* S = new R4State();
    m->r4 = S;
    const ishara_config& c = m->cfg;
    const int d = m->d, L = c.num_conv_conform_blocks, k = c.transformer_kernel_size;
    S->T0 = c.frames; S->F = c.features;
    const R4Dims D = r4_dims(S->T0, S->F, d);
    S->T1 = D.T1; S->F1 = D.F1; S->T2 = D.T2; S->F2 = D.F2; S->T3 = D.T3; S->Fr = D.Fr; S->Kp = D.Kp; S->Trec = 2 * S->T3;
    S->reduce = c.reduce_layer_index < L ? c.reduce_layer_index : L;
    S->recover = c.recover_layer_index < L ? c.recover_layer_index : L;
    S->w1 = m->addp("conv_subsample.sequential.0.weight", d, 9, true); S->b1 = m->addp("conv_subsample.sequential.0.bias", d, 0, true);
    S->w2 = m->addp("conv_subsample.sequential.2.conv.weight", d, 9, true); S->b2 = m->addp("conv_subsample.sequential.2.conv.bias", d, 0, true);
    S->Win = m->dense_named("input_proj.0.weight", "input_proj.0.bias", d * S->F2, d);
    S->site_in = m->nsites++;
    S->trw = m->addp("time_reduction_layer.sequential.0.conv.weight", 9, 0, true); S->trb = m->addp("time_reduction_layer.sequential.0.conv.bias", 1, 0, true);
    S->Wred = m->dense_named("time_reduction_proj.weight", "time_reduction_proj.bias", S->Fr, d);
    S->Wrec = m->dense_named("time_recover_layer.weight", "time_recover_layer.bias", d, d);
    const float factor = c.half_step_residual ? 0.5f : 1.0f;
    int Tl = S->T2, stage = 0;
    for (int idx = 0; idx < L; ++idx) {
        if (idx == S->reduce) { Tl = S->T3; stage = 1; }
        if (idx == S->recover) { Tl = S->Trec; stage = 2; }
        R4Layer Ly;
        Ly.T = Tl; Ly.stage = stage;
        Ly.wrapped = idx >= S->reduce && idx < S->recover;
        const std::string s = "layers." + std::to_string(idx) + (Ly.wrapped ? ".module" : "") + ".sequential";
        const std::string a = s + ".0.module.attention";
        RelMHSA& A = Ly.mha;
        A.u = m->addp(a + ".u_bias", d, 0, true); A.v = m->addp(a + ".v_bias", d, 0, true);
        A.Wq = m->dense_named(a + ".query_proj.weight", a + ".query_proj.bias", d, d);
        A.Wk = m->dense_named(a + ".key_proj.weight", a + ".key_proj.bias", d, d);
        A.Wv = m->dense_named(a + ".value_proj.weight", a + ".value_proj.bias", d, d);
        A.Wpos = m->dense_named(a + ".pos_proj.weight", "", d, d);
        A.Wo = m->dense_named(a + ".out_proj.weight", a + ".out_proj.bias", d, d);
        A.ln = m->norm_named(s + ".1", d);
        A.site_attn = m->nsites++; A.site_out = m->nsites++;
        Ly.ffn1 = r4_build_ffn(m, s + ".2.module", s + ".3", factor);
        ConfConv& cv = Ly.conv;
        const std::string cs = s + ".4.module.sequential";
        cv.k = k; cv.bn_eps = R4_EPS; cv.ln_eps = R4_EPS; cv.bn_keep = 0.9f; cv.bn_unbiased = 1; cv.swish_after_bn = 1; cv.has_out_drop = 1;
        cv.Wp1 = m->dense_named(cs + ".1.conv.weight", cs + ".1.conv.bias", d, 2 * d);
        cv.dw = m->addp(cs + ".3.conv.weight", k, d, true);
        cv.dwb = -1;
        cv.bn.gamma = m->addp(cs + ".4.weight", d, 0, true); cv.bn.beta = m->addp(cs + ".4.bias", d, 0, true);
        cv.bn.mm = m->addp(cs + ".4.running_mean", d, 0, false); cv.bn.mv = m->addp(cs + ".4.running_var", d, 0, false);
        cv.Wp2 = m->dense_named(cs + ".6.conv.weight", cs + ".6.conv.bias", d, d);
        cv.site_out = m->nsites++;
        cv.ln = m->norm_named(s + ".5", d);
        Ly.ffn2 = r4_build_ffn(m, s + ".6.module", s + ".7", factor);
        // the table this layer's length needs
        int pe = -1;
        for (size_t t = 0; t < S->pe_T.size(); ++t) if (S->pe_T[t] == Tl) pe = (int)t;
        if (pe < 0) { pe = (int)S->pe_T.size(); S->pe_T.push_back(Tl); }
        Ly.pe = pe;
        S->layers.push_back(Ly);
        m->layer_entry_end.push_back(m->entries.size());
    }
    S->Tout = Tl;
    finish_param_layout(m);
    m->bucket_lo.push_back(0); m->bucket_hi.push_back(m->n_train);
    m->bucket_after_layer.assign(S->layers.size(), -1);
    // R2: RelPositionalEncoding rows for T frames (modules.py:73-108): row r = relative position T-1-r, even columns sin, odd cos
    for (int T : S->pe_T) {
        std::vector<float> tab((size_t)(2 * T - 1) * d);
        for (int r = 0; r < 2 * T - 1; ++r) {
            const float pos = (float)(T - 1 - r);
            for (int i = 0; i < d; i += 2) {
                const float div = expf((float)i * -(logf(10000.0f) / (float)d));
                tab[(size_t)r * d + i] = sinf(pos * div);
                if (i + 1 < d) tab[(size_t)r * d + i + 1] = cosf(pos * div);
            }
        }
        S->pe_host.push_back(tab);
    }
}

void r4_plan_workspace(ishara_model* m) {
    R4State* S = m->r4;
    const int d = m->d, B = m->Bmax, de = d * m->cfg.expansion_factor;
    const size_t es = dt_size(m->dt);
    const int Tmax = S->T2 > S->Trec ? S->T2 : S->Trec;
    m->cur = 0;
    m->shadow_begin = m->cur;
    plan_shadow(m, S->Win); plan_shadow(m, S->Wred, S->Kp); plan_shadow(m, S->Wrec);
    for (auto& L : S->layers)
        for (DenseW* w : {&L.mha.Wq, &L.mha.Wk, &L.mha.Wv, &L.mha.Wpos, &L.mha.Wo, &L.ffn1.W1, &L.ffn1.W2, &L.conv.Wp1, &L.conv.Wp2, &L.ffn2.W1, &L.ffn2.W2}) plan_shadow(m, *w);
    m->shadow_end = m->cur;
    m->shadow_tab_off = m->alloc(m->denses.size() * sizeof(ShadowDesc)).off;
    S->y1 = m->f32((size_t)B * d * S->T1 * S->F1); S->dz1 = m->f32((size_t)B * d * S->T1 * S->F1);
    S->sub = m->alloc((size_t)B * S->T2 * d * S->F2 * es); S->dsub = m->alloc((size_t)B * S->T2 * d * S->F2 * es);
    S->h0 = m->alloc((size_t)B * S->T2 * d * es);
    S->trpre = m->f32((size_t)B * S->T3 * S->Fr); S->trout = m->alloc((size_t)B * S->T3 * S->Kp * es); S->red = m->alloc((size_t)B * S->T3 * d * es);
    S->rep = m->alloc((size_t)B * S->Trec * d * es); S->crop = m->alloc((size_t)B * S->Trec * d * es); S->rec = m->alloc((size_t)B * S->Trec * d * es);
    S->gskip = m->alloc((size_t)B * S->T2 * d * es); S->gwrap = m->alloc((size_t)B * Tmax * d * es);
    S->dqb = m->alloc((size_t)B * Tmax * d * es); S->dkb = m->alloc((size_t)B * Tmax * d * es); S->dvb = m->alloc((size_t)B * Tmax * d * es);
    S->dposp = m->f32((size_t)(2 * Tmax - 1) * d);
    S->dwred = m->f32((size_t)S->Kp * d);
    for (size_t t = 0; t < S->pe_T.size(); ++t) {
        S->pe32.push_back(m->f32((size_t)(2 * S->pe_T[t] - 1) * d));
        S->pedt.push_back(m->alloc((size_t)(2 * S->pe_T[t] - 1) * d * es));
    }
    for (auto& L : S->layers) {
        const size_t Mx = (size_t)B * L.T;
        auto A = [&](int cols) { return m->alloc(Mx * cols * es); };
        RelMHSA& a = L.mha;
        a.q = A(d); a.k = A(d); a.vv = A(d); a.o = A(d); a.lse = m->f32((size_t)B * m->H * L.T); a.posp = m->f32((size_t)(2 * L.T - 1) * d);
        a.r = A(d); a.mean = m->f32(Mx); a.rstd = m->f32(Mx); a.out = A(d);
        plan_post_ln_ffn(m, L.ffn1, Mx, d, de); plan_post_ln_ffn(m, L.ffn2, Mx, d, de);
        plan_confconv(m, L.conv, Mx, B, d);      // with sw (swish_after_bn)
        if (L.wrapped) L.wrap_out = A(d);
    }
    const size_t Mmax = (size_t)B * Tmax;
    const int maxw = de > 2 * d ? de : 2 * d;
    m->gA = m->alloc(Mmax * d * es); m->gB = m->alloc(Mmax * d * es); m->t4 = m->alloc(Mmax * d * es);
    m->t1 = m->alloc(Mmax * maxw * es); m->t2 = m->alloc(Mmax * maxw * es); m->t3 = m->alloc(Mmax * maxw * es);
    m->S1 = m->f32((size_t)B * maxw); m->S2 = m->f32((size_t)B * maxw); m->E = m->f32((size_t)B * maxw);
    m->Fc = m->f32(maxw); m->Ecol = m->f32(maxw); m->fac = m->f32(B);
    m->slab = m->f32(slab_floats(m, Mmax, B, Tmax, maxw, S->Kp));      // K at least Kp: the padded time_reduction_proj wgrad (r4_backward)
    m->delta = m->f32((size_t)B * m->H * Tmax);
    S->nlen = m->alloc((size_t)3 * B * sizeof(int));
    m->ws_need = m->cur;
}

int r4_bind(ishara_model* m) {
    R4State* S = m->r4;
    for (size_t t = 0; t < S->pe_T.size(); ++t)
        HIP_CHECK_RET(hipMemcpy(m->ws + S->pe32[t].off, S->pe_host[t].data(), S->pe_host[t].size() * sizeof(float), hipMemcpyHostToDevice));
    std::vector<float> fac((size_t)m->Bmax, m->cfg.half_step_residual ? 0.5f : 1.0f);
    HIP_CHECK_RET(hipMemcpy(m->ws + m->fac.off, fac.data(), fac.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
void r4_destroy(ishara_model* m) { delete m->r4; m->r4 = nullptr; }
int r4_output_frames(const ishara_model* m) { return m->r4->Tout; }

// ------------------------------------------------------------------ forward
static const void* r4_layer_out(ishara_model* m, const R4Layer& L) { return L.wrapped ? m->W(L.wrap_out) : m->W(L.ffn2.out); }
static int r4_mhsa_fwd(ishara_model* m, R4State* S, R4Layer& L, const Run& r, const void* x) {
    RelMHSA& a = L.mha;
    const int dt = m->dt, d = m->d, T = L.T;
    OpArgs no; EpiArgs e0;
    CK(gemm_fwd(m, a.Wq, x, dt, m->W(a.q), dt, r.M, OP_NONE, no, e0));
    CK(gemm_fwd(m, a.Wk, x, dt, m->W(a.k), dt, r.M, OP_NONE, no, e0));
    CK(gemm_fwd(m, a.Wv, x, dt, m->W(a.vv), dt, r.M, OP_NONE, no, e0));
    // pos_proj of the table (the reference repeats the table over the batch, attention.py:135; the projection does not depend on it)
    CK(gemm_fwd(m, a.Wpos, m->dt == DT_F32 ? (const void*)m->Wf(S->pe32[L.pe]) : (const void*)m->W(S->pedt[L.pe]), dt, m->Wf(a.posp), DT_F32, 2 * T - 1, OP_NONE, no, e0));
    const float scale = 1.0f / sqrtf((float)m->dh);
    CKP(m, "relattn_fwd", 4.0 * r.M * d * (double)dt_size(dt), 8.0 * r.B * m->H * (double)T * T * m->dh,
        launch_relattn_len_fwd(dt, m->W(a.q), m->W(a.k), m->W(a.vv), m->Wf(a.posp), m->P(a.u), m->P(a.v), m->W(a.o), m->Wf(a.lse), r.key_len, false, r.B, m->H, T, m->dh, scale,
                               dspec_attn(r, a.site_attn, m->cfg.dropout_rate), m->s));      // r.key_len: this layer's keys per clip (nullptr: every key)
    EpiArgs ep; ep.resid = x; ep.drop = dspec(r, a.site_out, m->cfg.dropout_rate);
    CK(gemm_fwd(m, a.Wo, m->W(a.o), dt, m->W(a.r), dt, r.M, OP_NONE, no, ep));
    return r5_ln_fwd(m, r, m->W(a.r), a.ln, m->W(a.out), a.mean, a.rstd);
}

int r4_forward(ishara_model* m, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, hipStream_t st, const int32_t* input_len) {
    R4State* S = m->r4;
    m->s = st;
    int* nlen = nullptr;      // masked pass: the keys per clip of the three attention resolutions, on the device
    if (input_len) { nlen = m->W<int>(S->nlen); CK(r4_stage_len_launch(input_len, nlen, B, S->T0, S->T2, S->T3, S->Trec, m->s)); }
    const int dt = m->dt, d = m->d;
    OpArgs no;
    Run r{B, B * S->T2, training, seed};
    // tables in the storage type (A operand of the pos_proj GEMM)
    if (dt != DT_F32)
        for (size_t t = 0; t < S->pe_T.size(); ++t) CK(r5_from_f32(dt, m->Wf(S->pe32[t]), m->W(S->pedt[t]), (size_t)(2 * S->pe_T[t] - 1) * d, m->s));
    // ---- DepthwiseConv2dSubsampling + input_proj (encoder.py:148-149)
    CK(r4_subsample_fwd_launch(dt, x, m->P(S->w1), m->P(S->b1), m->P(S->w2), m->P(S->b2), m->Wf(S->y1), m->W(S->sub), B, S->T0, S->F, d, S->T1, S->F1, S->T2, S->F2, m->s));
    EpiArgs ein; ein.drop = dspec(r, S->site_in, m->cfg.dropout_rate);
    CK(gemm_fwd(m, S->Win, m->W(S->sub), dt, m->W(S->h0), dt, r.M, OP_NONE, no, ein));
    const void* h = m->W(S->h0);
    const void* recover_src = nullptr;
    const int keepT = m->T;
    int Tl = S->T2;
    for (int idx = 0; idx < (int)S->layers.size(); ++idx) {
        R4Layer& L = S->layers[idx];
        if (idx == S->reduce) {            // time reduction (encoder.py:152-155)
            recover_src = h;
            CK(r4_tred_fwd_launch(dt, h, m->P(S->trw), m->P(S->trb), m->Wf(S->trpre), m->W(S->trout), B, Tl, d, S->T3, S->Fr, S->Kp, m->s));
            DenseW wp = S->Wred; wp.K = S->Kp;
            EpiArgs e0;
            CK(gemm_fwd(m, wp, m->W(S->trout), dt, m->W(S->red), dt, B * S->T3, OP_NONE, no, e0));
            h = m->W(S->red); Tl = S->T3;
        }
        if (idx == S->recover) {           // recover_resolution + Linear + skip (encoder.py:157-162)
            CK(r4_rows_mode_launch(dt, R4_ROWS_RECOVER, h, nullptr, m->W(S->rep), B, S->Trec, S->T3, d, m->s));
            CK(r4_rows_mode_launch(dt, R4_ROWS_CROP, recover_src, nullptr, m->W(S->crop), B, S->Trec, S->T2, d, m->s));
            EpiArgs er; er.resid = m->W(S->crop);
            CK(gemm_fwd(m, S->Wrec, m->W(S->rep), dt, m->W(S->rec), dt, B * S->Trec, OP_NONE, no, er));
            h = m->W(S->rec); Tl = S->Trec;
        }
        m->T = Tl;
        Run rl{B, B * Tl, training, seed};
        Run ra = rl; ra.key_len = nlen ? nlen + L.stage * B : nullptr;      // only the attention sees the lengths
        CK(r4_mhsa_fwd(m, S, L, ra, h));
        CK(r5_ffn_fwd(m, L.ffn1, rl, m->W(L.mha.out)));
        CK(confconv_fwd(m, L.conv, rl, m->W(L.ffn1.out)));
        CK(r5_ffn_fwd(m, L.ffn2, rl, m->W(L.conv.out)));
        const void* out = m->W(L.ffn2.out);
        if (L.wrapped) { CK(r4_rows_mode_launch(dt, R4_ROWS_ADD, h, out, m->W(L.wrap_out), B, Tl, Tl, d, m->s)); out = m->W(L.wrap_out); }      // ResidualConnectionModule around the block
        h = out;
    }
    m->T = keepT;
    CK(r5_to_f32(dt, h, y, (size_t)B * S->Tout * d, m->s));
    m->lastB = B; m->last_training = training; m->last_seed = seed; m->last_x = x;
    return 0;
}

// ------------------------------------------------------------------ backward
static int r4_mhsa_bwd(ishara_model* m, R4State* S, R4Layer& L, const Run& r, const void* x, const void* g, void* gn) {
    RelMHSA& a = L.mha;
    const int dt = m->dt, d = m->d, T = L.T;
    OpArgs no; EpiArgs e0;
    void* dr = m->W(m->t4);
    CK(r5_ln_bwd(m, r, g, m->W(a.r), a.ln, a.mean, a.rstd, dr));
    int rc = 0;
    const void* gs = grad_through_dropout(m, r, a.site_out, m->cfg.dropout_rate, dr, m->W(m->t3), T, d, &rc);
    CK(rc);
    CK(gemm_dgrad(m, a.Wo, gs, dt, m->W(m->t1), r.M, OP_NONE, no, e0));                          // d context
    CK(gemm_wgrad(m, a.Wo, m->W(a.o), dt, OP_NONE, no, gs, dt, OP_NONE, no, r.M));
    CK(r4_fill_f32_launch(m->Wf(S->dposp), (size_t)(2 * T - 1) * d, 0.f, m->s));
    const float scale = 1.0f / sqrtf((float)m->dh);
    CKP(m, "relattn_bwd", 12.0 * r.M * d * (double)dt_size(dt), 24.0 * r.B * m->H * (double)T * T * m->dh,
        launch_relattn_len_bwd(dt, m->W(a.q), m->W(a.k), m->W(a.vv), m->Wf(a.posp), m->P(a.u), m->P(a.v), m->W(a.o), m->W(m->t1), m->Wf(a.lse), m->Wf(m->delta),
                               m->W(S->dqb), m->W(S->dkb), m->W(S->dvb), m->G(a.u), m->G(a.v), m->Wf(S->dposp), r.key_len, r.B, m->H, T, m->dh, scale,
                               dspec_attn(r, a.site_attn, m->cfg.dropout_rate), m->s));
    // pos_proj weight gradient: table^T . dposp (no bias, the table itself has no gradient)
    CK(gemm_wgrad(m, a.Wpos, m->dt == DT_F32 ? (const void*)m->Wf(S->pe32[L.pe]) : (const void*)m->W(S->pedt[L.pe]), dt, OP_NONE, no, m->Wf(S->dposp), DT_F32, OP_NONE, no, 2 * T - 1));
    // the three input projections: dx = dr + dq Wq^T + dk Wk^T + dv Wv^T
    EpiArgs e1; e1.resid = dr;
    CK(gemm_dgrad(m, a.Wq, m->W(S->dqb), dt, m->W(m->t1), r.M, OP_NONE, no, e1));
    EpiArgs e2; e2.resid = m->W(m->t1);
    CK(gemm_dgrad(m, a.Wk, m->W(S->dkb), dt, m->W(m->t2), r.M, OP_NONE, no, e2));
    EpiArgs e3; e3.resid = m->W(m->t2);
    CK(gemm_dgrad(m, a.Wv, m->W(S->dvb), dt, gn, r.M, OP_NONE, no, e3));
    CK(gemm_wgrad(m, a.Wq, x, dt, OP_NONE, no, m->W(S->dqb), dt, OP_NONE, no, r.M));
    CK(gemm_wgrad(m, a.Wk, x, dt, OP_NONE, no, m->W(S->dkb), dt, OP_NONE, no, r.M));
    CK(gemm_wgrad(m, a.Wv, x, dt, OP_NONE, no, m->W(S->dvb), dt, OP_NONE, no, r.M));
    return 0;
}

int r4_backward(ishara_model* m, const float* dy, int32_t B, float* dx, hipStream_t st, const int32_t* input_len) {
    R4State* S = m->r4;
    m->s = st;
    int* nlen = nullptr;      // derived again from the caller's array: the library keeps no pointer between the two calls
    if (input_len) { nlen = m->W<int>(S->nlen); CK(r4_stage_len_launch(input_len, nlen, B, S->T0, S->T2, S->T3, S->Trec, m->s)); }
    const int dt = m->dt, d = m->d;
    OpArgs no; EpiArgs e0;
    CK(launch_fill_u32(m->grads, (size_t)m->n_train, 0u, m->s));
    void* g = m->W(m->gA); void* gn = m->W(m->gB);
    // gradient of the output in the storage type
    if (dt != DT_F32) CK(r5_from_f32(dt, dy, g, (size_t)B * S->Tout * d, m->s));
    else HIP_CHECK_RET(hipMemcpyAsync(g, dy, (size_t)B * S->Tout * d * sizeof(float), hipMemcpyDeviceToDevice, m->s));
    const int keepT = m->T;
    bool have_skip = false;
    // inputs of the layers, as the forward pass chained them
    std::vector<const void*> lin(S->layers.size());
    {
        const void* h = m->W(S->h0);
        for (int idx = 0; idx < (int)S->layers.size(); ++idx) {
            if (idx == S->reduce) h = m->W(S->red);
            if (idx == S->recover) h = m->W(S->rec);
            lin[idx] = h;
            h = r4_layer_out(m, S->layers[idx]);
        }
    }
#define SWAP() do { void* _t = g; g = gn; gn = _t; } while (0)
    for (int idx = (int)S->layers.size() - 1; idx >= 0; --idx) {
        R4Layer& L = S->layers[idx];
        const int Tl = L.T;
        m->T = Tl;
        Run rl{B, B * Tl, 1, m->last_seed};
        Run ra = rl; ra.key_len = nlen ? nlen + L.stage * B : nullptr;
        if (L.wrapped) HIP_CHECK_RET(hipMemcpyAsync(m->W(S->gwrap), g, (size_t)rl.M * d * dt_size(dt), hipMemcpyDeviceToDevice, m->s));   // the skip branch of the wrapper
        CK(r5_ffn_bwd(m, L.ffn2, rl, m->W(L.conv.out), g, gn)); SWAP();
        CK(confconv_bwd(m, L.conv, rl, m->W(L.ffn1.out), g, gn)); SWAP();
        CK(r5_ffn_bwd(m, L.ffn1, rl, m->W(L.mha.out), g, gn)); SWAP();
        CK(r4_mhsa_bwd(m, S, L, ra, lin[idx], g, gn)); SWAP();
        if (L.wrapped) { CK(r4_rows_mode_launch(dt, R4_ROWS_ADD, m->W(S->gwrap), g, gn, B, Tl, Tl, d, m->s)); SWAP(); }
        if (idx == S->recover) {           // g = gradient of rec = Linear(rep) + crop(recover_src)
            CK(r4_rows_mode_launch(dt, R4_ROWS_CROP_BWD, g, nullptr, m->W(S->gskip), B, S->T2, S->Trec, d, m->s));        // into the longer pre-reduction sequence
            have_skip = true;
            CK(gemm_dgrad(m, S->Wrec, g, dt, m->W(m->t1), B * S->Trec, OP_NONE, no, e0));
            CK(gemm_wgrad(m, S->Wrec, m->W(S->rep), dt, OP_NONE, no, g, dt, OP_NONE, no, B * S->Trec));
            CK(r4_rows_mode_launch(dt, R4_ROWS_RECOVER_BWD, m->W(m->t1), nullptr, gn, B, S->T3, S->Trec, d, m->s)); SWAP();
        }
        if (idx == S->reduce) {            // g = gradient of red = Linear(swish(conv3x3(h)))
            DenseW wp = S->Wred; wp.K = S->Kp;
            CK(gemm_dgrad(m, wp, g, dt, m->W(m->t1), B * S->T3, OP_NONE, no, e0));                    // d trout [B*T3, Kp]
            CKP(m, "wgrad(time_reduction_proj)", 0, 0, r4_tred_wgrad_launch(dt, m->W(S->trout), g, m->Wf(S->dwred), m->G(S->Wred.w), m->G(S->Wred.b), m->Wf(m->slab), B * S->T3, S->Fr, S->Kp, d, m->s));
            const void* hprev = idx > 0 ? r4_layer_out(m, S->layers[idx - 1]) : m->W(S->h0);
            CK(r4_tred_bwd_launch(dt, m->W(m->t1), m->Wf(S->trpre), hprev, m->P(S->trw), have_skip ? m->W(S->gskip) : nullptr, m->G(S->trw), m->G(S->trb), gn, B, S->T2, d, S->T3, S->Fr, S->Kp, m->s));
            SWAP();
        }
    }
#undef SWAP
    m->T = keepT;
    // ---- input_proj and the convolution subsampling
    Run r0{B, B * S->T2, 1, m->last_seed};
    int rc = 0;
    const void* gs = grad_through_dropout(m, r0, S->site_in, m->cfg.dropout_rate, g, gn, S->T2, d, &rc);
    CK(rc);
    CK(gemm_wgrad(m, S->Win, m->W(S->sub), dt, OP_NONE, no, gs, dt, OP_NONE, no, r0.M));
    CK(gemm_dgrad(m, S->Win, gs, dt, m->W(S->dsub), r0.M, OP_NONE, no, e0));
    CK(r4_subsample_bwd_launch(dt, m->W(S->dsub), m->W(S->sub), m->Wf(S->y1), m->last_x, m->P(S->w1), m->P(S->w2), m->Wf(S->dz1), m->G(S->w1), m->G(S->b1), m->G(S->w2), m->G(S->b2), dx,
                               B, S->T0, S->F, d, S->T1, S->F1, S->T2, S->F2, m->s));
    if (!m->bucket_ev.empty()) HIP_CHECK_RET(hipEventRecord(m->bucket_ev.back(), m->s));
    return 0;
}

// ------------------------------------------------------------------ the call with per-clip input lengths
// ishara_encoder_forward_lengths / _backward_lengths: the padding mask of this family.  input_len device int32 [B], input frames per clip; the keys
// of every attention layer at or past the clip's length AT THAT LAYER'S RESOLUTION are masked (r4_stage_len_launch), nothing else changes.
// input_len NULL is ishara_encoder_forward / _backward, on the same kernels.  Every check is made before any GPU work
static int r4_lengths_refused(const char* me, const ishara_model* m, const int32_t* input_len) {
    if (m->family == ISHARA_FAMILY_TORCH_CONFORMER) { ishara_set_error("%s: input lengths are served by ISHARA_FAMILY_TORCH_SQUEEZEFORMER only: the Conformer encoder takes key_len of ishara_encoder_forward_ex", me); return -1; }
    if (m->family != ISHARA_FAMILY_TORCH_SQUEEZEFORMER) { ishara_set_error("%s: input lengths are served by ISHARA_FAMILY_TORCH_SQUEEZEFORMER only: the Keras hybrid takes frame_len of ishara_forward_ex", me); return -1; }
    if (m->dt == DT_F16) { ishara_set_error("%s: ISHARA_F16 is refused: the torch Squeezeformer family has no fp16 kernels", me); return -1; }
    if (input_len && (uintptr_t)input_len % 4) { ishara_set_error("%s: misaligned input_len: an int32 array", me); return -1; }
    return 0;
}
extern "C" int ishara_encoder_forward_lengths(ishara_model* m, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, const int32_t* input_len, ishara_stream st) {
    const char* me = "ishara_encoder_forward_lengths";
    if (r4_lengths_refused(me, m, input_len)) return -1;
    if (!m->ws) { ishara_set_error("%s: model is not bound", me); return -1; }
    if (B <= 0 || B > m->Bmax) { ishara_set_error("%s: batch %d outside 1..%d", me, B, m->Bmax); return -1; }
    m->last_masked = input_len ? 1 : 0;
    return r4_forward(m, x, B, y, training, seed, (hipStream_t)st, input_len);
}
extern "C" int ishara_encoder_backward_lengths(ishara_model* m, const float* dy, int32_t B, float* dx, const int32_t* input_len, ishara_stream st) {
    const char* me = "ishara_encoder_backward_lengths";
    if (r4_lengths_refused(me, m, input_len)) return -1;
    if (!m->ws || !m->grads) { ishara_set_error("%s: model is not bound (grads required)", me); return -1; }
    if (B != m->lastB || !m->last_training) { ishara_set_error("%s: call ishara_encoder_forward(training=1) with the same batch first", me); return -1; }
    const bool masked = input_len != nullptr;
    if (masked != (m->last_masked != 0)) {
        ishara_set_error("%s: the last training forward pass was %s an attention mask and this call is %s one: pass the same input_len array again", me,
                         m->last_masked ? "given" : "not given", masked ? "given" : "not given");
        return -1;
    }
    return r4_backward(m, dy, B, dx, (hipStream_t)st, input_len);
}
