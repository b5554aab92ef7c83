// The Conv1DBlock of the Keras get_model hybrid (conv-hybrid-model.ipynb c5:60-88): expand Dense -> Swish -> causal depthwise conv -> BatchNorm -> ECA
// gate -> project Dense (+ drop-path, + residual).  conv_block_plan states once which launches a block's forward and backward run; conv_fwd and
// conv_bwd are switches over that plan.  The two launch pairs a Conformer conv module shares with the block (depthwise forward + BatchNorm
// constants, BatchNorm backward carried by the depthwise backward) are here too: confconv_fwd / _bwd (keras_hybrid.hip) call them.
#include "model_types.h"
#include <stdlib.h>

// ---- the fusion switches: read here and nowhere else
bool infer_fusion_on() { return getenv("ISHARA_NO_INFER_FUSION") == nullptr; }      // at every call that asks (conv_block_plan at inference, cls_route_auto)
bool stats_fusion_on() { static const bool on = getenv("ISHARA_NO_STATS_FUSION") == nullptr; return on; }      // once per process
static int psa_dbg() { static const int v = getenv("ISHARA_PSA_DBG") ? atoi(getenv("ISHARA_PSA_DBG")) : 0; return v; }      // ablation bits of the TnPsa weight gradient
int dwconv_stat_rows(int dt, int B, int T, int C, int k) { return dwconv_fwd_part_rows(dwconv_fwd_route(dt, B, T, C, k, true, true), B, T, C); }

// ---- The launch plan of one Conv1DBlock call, decided here and nowhere else: conv_fwd stores it in the ConvBlock, conv_bwd reads it back, and
// conv_block_route_name names it.  Inputs are plain values (ldt / ldn: the row strides of the project conv's two weight shadows, shadow_ld).
//   stats         which statistics the ECA gate reads (ConvStats)            bn_from_part  BatchNorm constants from the partial rows, not from per-sample sums
//   fold          the drop-path scale rs[b] is folded into P, Q (h4 = rs[b] * (h2 P + Q)), the GEMM adds rs[b] * b2, and the backward needs no scaled copy
//   prologue      h4 = h2 P[b] + Q[b] as an operand prologue of the project GEMM; else sample_affine + GEMM
//   psa           the project conv's weight gradient applies P, Q itself and emits the BatchNorm / ECA backward statistics: h4 is never written
//                 (gemm_tn.hip TnPsa: whole samples per M-split, all-T sums; a drop-path scale must be the folded one)
//   w2_bwd / bn_bwd   the project conv's gradient pair and the BatchNorm + depthwise backward (ConvW2Bwd, ConvBnBwd)
// A new form gets an enumerator or a field, its condition here, one case in the switches of conv_fwd / conv_bwd and a token in the name.
ConvPlan conv_block_plan(int dt, bool training, int B, int T, int d, int k, int ldt, int ldn, bool drop_path, bool lengths, bool psa_on) {
    ConvPlan p;
    const int c = 2 * d, M = B * T;
    p.prows = dwconv_stat_rows(dt, B, T, c, k);
    if (p.prows <= 0) return p;                          // the depthwise conv refuses (C, k)
    p.ok = true;
    p.bn_from_part = training && stats_fusion_on();
    p.stats = lengths ? ST_LEN : (!training && infer_fusion_on()) ? ST_INFER_PART : p.bn_from_part ? ST_TRAIN_PART : ST_SUMS;
    // the applicability tests look at an EpiArgs pointer only to see whether it is set: `set` stands for the buffers of the call
    const float* const set = reinterpret_cast<const float*>(uintptr_t(256));
    EpiArgs e; e.resid = set; e.bias = set;
    if (drop_path) {
        e.rowscale = set; e.T = T;
        p.fold = dt == DT_BF16 && !g_force_regstage && gemm_nt_as_applicable(dt, M, d, c, ldt, e) && gemm_nt_as_applicable(dt, M, c, d, ldn, e) && gemm_tn_bias_rowscale_ok(dt, dt, dt, M, c, d, T);
    }
    e.pa_P = set; e.pa_Q = set; e.T = T;
    p.prologue = gemm_nt_as_prologue_ok(dt, dt, dt, M, d, c, ldt, e);
    p.psa = p.prologue && training && psa_on && !lengths && (!drop_path || p.fold) && gemm_tn_psa_ok(dt, dt, dt, M, c, d, T);
    p.w2_bwd = p.psa ? W2_PSA : !drop_path ? W2_PLAIN : p.fold ? W2_FOLDED : W2_SCALED_COPY;
    // (the parameter-gradient scratch is always there: red_scratch falls back to the slab)
    p.bn_bwd = lengths ? BNB_LEN : dwconv_bwd_route(dt, c, k, k - 1, true, true).kind == DWB_FUSED_BN ? BNB_FUSED : BNB_TWO_KERNEL;
    return p;
}
// "forward|backward", e.g. "part+fold+prologue+psa|psa+fused_bn"; "" for a refused plan.  Valid until this thread's next call.
//   forward:  the BatchNorm constants' source (part | sums | infer: none, the gate forms them), "+len" for the length gate, "+fold", "+prologue" | "+affine", "+psa"
//   backward: psa | folded | scaled_copy | plain, then len | fused_bn | two_kernel; "-" at inference
const char* conv_block_route_name(const ConvPlan& p, bool training) {
    static thread_local char name[96];
    if (!p.ok) return "";
    static const char* const w2[] = {"psa", "folded", "scaled_copy", "plain"};      // by ConvW2Bwd
    static const char* const bnb[] = {"len", "fused_bn", "two_kernel"};             // by ConvBnBwd
    const int n = snprintf(name, sizeof name, "%s%s%s%s%s|", p.stats == ST_INFER_PART ? "infer" : (p.bn_from_part ? "part" : "sums"), p.stats == ST_LEN ? "+len" : "",
                           p.fold ? "+fold" : "", p.prologue ? "+prologue" : "+affine", p.psa ? "+psa" : "");
    if (training) snprintf(name + n, sizeof name - n, "%s+%s", w2[p.w2_bwd], bnb[p.bn_bwd]);
    else snprintf(name + n, sizeof name - n, "-");
    return name;
}

// ---- shared pair 1: the depthwise conv and the BatchNorm constants of its output.  prows > 0: the conv leaves that many partial statistic rows per
// sample in the slab and the constants come straight from them (no stats_reduce launch); 0: per-sample sums in s.ssum / s.ssq (with_sums: wanted
// at all — a Conformer conv at inference reads the moving statistics only).  finalize = false: no bn_finalize (the inference gate forms the constants).
int dwconv_bn_fwd(ishara_model* m, const Run& r, int inop, const void* x, int dw, int dwb, void* y, int C, int k, int padl, const DwBnFwd& s, bool with_sums, int prows, bool finalize) {
    const int B = r.B, T = m->T;
    int got = 0;
    CKP(m, "dwconv_fwd", 3.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_dwconv_fwd(m->dt, inop, x, m->P(dw), dwb >= 0 ? m->P(dwb) : nullptr, y, with_sums ? m->Wf(s.ssum) : nullptr, with_sums ? m->Wf(s.ssq) : nullptr,
                                                                                          m->Wf(m->slab), B, T, C, k, padl, m->s, prows ? &got : nullptr));
    if (got != prows) { ishara_set_error("dwconv_bn_fwd: internal error: %d partial rows planned, %d written (C=%d k=%d)", prows, got, C, k); return -2; }
    if (!finalize) return 0;
    if (prows)       // batch statistics straight from the partial rows [B * prows][2][C]
    CKP(m, "bn_finalize", 0, 0, launch_bn_finalize(m->Wf(m->slab), m->Wf(m->slab) + C, B * prows, (float)B * T, m->P(s.bn.gamma), m->P(s.bn.beta), s.eps, s.keep,
                          m->P(s.bn.mm), m->P(s.bn.mv), r.training, m->Wf(s.mean), m->Wf(s.rstd), m->Wf(s.a), m->Wf(s.bsh), C, m->s, s.var_corr, 2 * C));
    else
    CKP(m, "bn_finalize", 0, 0, launch_bn_finalize(m->Wf(s.ssum), m->Wf(s.ssq), B, (float)B * T, m->P(s.bn.gamma), m->P(s.bn.beta), s.eps, s.keep,
                          m->P(s.bn.mm), m->P(s.bn.mv), r.training, m->Wf(s.mean), m->Wf(s.rstd), m->Wf(s.a), m->Wf(s.bsh), C, m->s, s.var_corr));
    return 0;
}
// ---- shared pair 2: the BatchNorm backward carried by the depthwise-conv backward.  fused (dwconv_bwd_fused_bn: what dwconv_bwd_route answers for
// the shape): one pass over dy, bn.h and x, booked as by_fused passes over [M, d]; else bn_bwd_apply on dy in place, then the plain backward.
bool dwconv_bwd_fused_bn(int dt, int C, int k, int padl) { return dwconv_bwd_route(dt, C, k, padl, true, true).kind == DWB_FUSED_BN; }
int dwconv_bn_bwd(ishara_model* m, const Run& r, bool fused, double by_fused, int inop, void* dy, const DwBnArgs& bn, const void* x, int dw, int dwb, void* dx, int C, int k, int padl) {
    if (fused) {
        const int rc = dwconv_bwd_deferred(m, r, by_fused, inop, dy, &bn, x, dw, dwb, dx, C, k, padl);
        if (rc == 0) { ishara_set_error("dwconv_bn_bwd: internal error: the fused BatchNorm / depthwise backward the plan chose refused the call (C=%d k=%d)", C, k); return -2; }
        return rc < 0 ? rc : 0;
    }
    CKP(m, "bn_bwd_apply", 6.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_bn_bwd_apply(m->dt, dy, bn.h, bn.mean, bn.rstd, bn.a, bn.sg, bn.E, bn.e_per_sample, bn.Fc, dy, r.B, m->T, C, m->s));
    CK(dwconv_bwd_deferred(m, r, 8.0, inop, dy, nullptr, x, dw, dwb, dx, C, k, padl));
    return 0;
}

// ------------------------------------------------------------------ module forward
int conv_fwd(ishara_model* m, ConvBlock& cb, const Run& r, const void* x) {
    const int d = m->d, c = 2 * d, B = r.B, T = m->T, dt = m->dt;
    OpArgs no; EpiArgs e1;
    // Frame lengths (r.key_len; DESIGN §2 "Frame lengths"): the ECA gate pools BN(h2) over the clip's n_b valid frames (c5:8-9).  BatchNorm's statistics
    // stay over all B*T rows, so the depthwise conv's statistics pass runs as without lengths; a masked time mean of h2 (a kernel of its own) then
    // feeds eca_fwd_len (g = 0 at n_b = 0).
    const int* fl = r.key_len;
    // Drop-path (c5:82-83) on the branch: y = x + rs[b] * (h4 W2 + b2); rs[b] itself is drawn by eca_fwd below (one launch less per block)
    const DropSpec ds = dspec(r, cb.site, m->cfg.dropout_rate);
    const ConvPlan p = cb.plan = conv_block_plan(dt, r.training != 0, B, T, d, cb.k, cb.W2.ldt, cb.W2.ldn, ds.thr != 0, fl != nullptr, m->psa_on);      // (!p.ok: launch_dwconv_fwd refuses and says why)
    float* rs = ds.thr ? m->Wf(cb.rs) : nullptr;
    float *gn = m->Wf(cb.gn), *sg = m->Wf(cb.sg), *P = m->Wf(cb.P), *Q = m->Wf(cb.Q), *part = m->Wf(m->slab);
    CK(gemm_fwd(m, cb.W1, x, dt, m->W(cb.z1), dt, r.M, OP_NONE, no, e1));
    const DwBnFwd st = {cb.bn, 1e-3f, 0.95f, 1.f, cb.ssum, cb.ssq, cb.mean, cb.rstd, cb.a, cb.bsh};
    CK(dwconv_bn_fwd(m, r, DWIN_SWISH, m->W(cb.z1), cb.dw, -1, m->W(cb.h2), c, cb.k, cb.k - 1, st, true, (p.bn_from_part || p.stats == ST_INFER_PART) ? p.prows : 0, p.stats != ST_INFER_PART));
    switch (p.stats) {
    case ST_LEN:
        CKP(m, "masked_time_mean", 1.0 * r.M * c * (double)dt_size(dt), 0, launch_masked_time_mean(dt, m->W(cb.h2), fl, m->Wf(cb.ssum), B, T, c, m->s));
        CKP(m, "eca_fwd_len", 0, 0, launch_eca_fwd_len(m->Wf(cb.ssum), m->Wf(cb.a), m->Wf(cb.bsh), m->P(cb.eca), fl, T, gn, sg, P, Q, B, c, m->s, rs, ds, p.fold));
        break;
    case ST_INFER_PART:      // the partial rows are summed, and the BatchNorm constants formed from the moving statistics, inside the gate kernel (4 launches per
        // Conv1DBlock instead of 6: at B = 1 every launch is ~9 us of latency)
        CKP(m, "eca_fwd", 0, 0, launch_eca_fwd_infer(part, p.prows, m->P(cb.bn.mm), m->P(cb.bn.mv), m->P(cb.bn.gamma), m->P(cb.bn.beta), 1e-3f, m->P(cb.eca), 1.f / T, gn, sg, P, Q, B, c, m->s));
        break;
    case ST_TRAIN_PART:      // the gate sums the partial rows per sample
        CKP(m, "eca_fwd", 0, 0, launch_eca_fwd_part(part, p.prows, m->Wf(cb.ssum), m->Wf(cb.a), m->Wf(cb.bsh), m->P(cb.eca), 1.f / T, gn, sg, P, Q, B, c, m->s, rs, ds, p.fold));
        break;
    case ST_SUMS:
        CKP(m, "eca_fwd", 0, 0, launch_eca_fwd(m->Wf(cb.ssum), m->Wf(cb.a), m->Wf(cb.bsh), m->P(cb.eca), 1.f / T, gn, sg, P, Q, B, c, m->s, rs, ds, p.fold));
        break;
    }
    EpiArgs e2; e2.resid = x;
    if (rs) { e2.rowscale = rs; e2.T = T; e2.rowscale_bias = p.fold; }
    const void* a2 = m->W(cb.h2);
    if (p.prologue) {      // h2 is read once; h4 is written from the transformed fragments, and only when the backward pass needs it in memory
        e2.pa_P = P; e2.pa_Q = Q; e2.T = T; e2.pro_out = (r.training && !p.psa) ? m->W(cb.h4) : nullptr;
    } else {
        CKP(m, "sample_affine", 4.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_affine(dt, m->W(cb.h2), P, Q, nullptr, m->W(cb.h4), B, T, c, m->s));
        a2 = m->W(cb.h4);
    }
    CK(gemm_fwd(m, cb.W2, a2, dt, m->W(cb.out), dt, r.M, OP_NONE, no, e2));
    return 0;
}

// ------------------------------------------------------------------ module backward: consumes g (grad wrt the module output), writes gn (grad wrt x)
int conv_bwd(ishara_model* m, ConvBlock& cb, const Run& r, const void* x, const void* g, void* gn) {
    const int d = m->d, c = 2 * d, B = r.B, T = m->T, dt = m->dt;
    OpArgs no;
    const ConvPlan& p = cb.plan;                         // of the training forward this backward belongs to
    const DropSpec ds = dspec(r, cb.site, m->cfg.dropout_rate);
    float* rs = ds.thr ? m->Wf(cb.rs) : nullptr;
    EpiArgs e1;
    if (rs && p.w2_bwd != W2_SCALED_COPY) { e1.rowscale = rs; e1.T = T; }      // dh4 = (g W2^T) * rs[b]: the dgrad scales its output rows
    switch (p.w2_bwd) {
    case W2_PSA: {       // h4 was never written: dW2 = sum_b diag(P_b) h2_b^T g_b + Q_b x colsum(g_b) inside the GEMM, which also emits the statistics of dh4
        CK(gemm_dgrad(m, cb.W2, g, dt, m->W(m->t1), r.M, OP_NONE, no, e1));      // (S1, S2 below) — no pass over dh4 and h2
        TnPsa ps; ps.P = m->Wf(cb.P); ps.Q = m->Wf(cb.Q); ps.W = m->ws + cb.W2.wn; ps.ldw = cb.W2.ldn; ps.G = m->Wf(m->psaG); ps.Rpart = m->Wf(m->psaR); ps.T = T;
        ps.dbg = psa_dbg();
        CK(gemm_wgrad(m, cb.W2, m->W(cb.h2), dt, OP_NONE, no, g, dt, OP_NONE, no, r.M, 0, 0, rs, rs ? T : 0, &ps));
        break; }
    case W2_FOLDED:      // h4 carries rs[b] (conv_fwd): dW2 = h4^T g; db2 = sum_m rs[b(m)] g[m]
        CK(gemm_dgrad(m, cb.W2, g, dt, m->W(m->t1), r.M, OP_NONE, no, e1));
        CK(gemm_wgrad(m, cb.W2, m->W(cb.h4), dt, OP_NONE, no, g, dt, OP_NONE, no, r.M, 0, 0, rs, T));
        break;
    case W2_SCALED_COPY:      // gradient through the drop-path: dY * rs[b]
        CKP(m, "map_rows", 2.0 * r.M * d * (double)dt_size(m->dt), 0, launch_map_rows(dt, MAP_ROWSCALE, g, m->W(m->t3), rs, ds, r.M, T, d, m->s));
        CK(gemm_dgrad(m, cb.W2, m->W(m->t3), dt, m->W(m->t1), r.M, OP_NONE, no, e1));
        CK(gemm_wgrad(m, cb.W2, m->W(cb.h4), dt, OP_NONE, no, m->W(m->t3), dt, OP_NONE, no, r.M));
        break;
    case W2_PLAIN:
        CK(gemm_dgrad(m, cb.W2, g, dt, m->W(m->t1), r.M, OP_NONE, no, e1));                       // dh4
        CK(gemm_wgrad(m, cb.W2, m->W(cb.h4), dt, OP_NONE, no, g, dt, OP_NONE, no, r.M));
        break;
    }
    PsaStats pst;                                        // W2_PSA: S1, S2 come out of the finalize kernel itself (from G and Rpart)
    if (p.psa) { pst.G = m->Wf(m->psaG); pst.Rpart = m->Wf(m->psaR); pst.nparts = cb.W2.N / 64; pst.Wt = m->ws + cb.W2.wt; pst.ldt = cb.W2.ldt; pst.N = cb.W2.N;
                 pst.rs = rs; pst.mean = m->Wf(cb.mean); pst.rstd = m->Wf(cb.rstd); }
    else CKP(m, "sample_reduce", 2.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_sample_reduce(dt, m->W(m->t1), m->W(cb.h2), m->Wf(cb.mean), m->Wf(cb.rstd), m->Wf(m->S1), m->Wf(m->S2), B, T, c, m->s));
    CKP(m, "eca_bn_bwd_finalize", 0, 0, launch_eca_bn_bwd_finalize(m->Wf(m->S1), m->Wf(m->S2), m->Wf(cb.ssum), m->Wf(cb.gn), m->Wf(cb.sg), m->P(cb.eca), m->P(cb.bn.gamma), m->P(cb.bn.beta),
                                  m->Wf(cb.mean), m->Wf(cb.rstd), m->G(cb.bn.gamma), m->G(cb.bn.beta), m->G(cb.eca), m->Wf(m->E), m->Wf(m->Fc), m->Wf(m->ecap), B, T, c, m->s, p.psa ? &pst : nullptr, r.key_len, m->Wf(m->Ecol)));
    if (p.bn_bwd == BNB_LEN) {      // frame lengths: the gate's gradient E[b,c] = dgn / n_b reaches the frames t < n_b only, Ecol[c] = -dbeta / Mtot every frame: a
        // two-kernel path, since the BatchNorm-carrying depthwise backward takes one constant per (sample, channel) (DESIGN §2 "Frame lengths": routes)
        CKP(m, "bn_bwd_apply_len", 6.0 * r.M * m->d * (double)dt_size(m->dt), 0, launch_bn_bwd_apply_len(dt, m->W(m->t1), m->W(cb.h2), m->Wf(cb.mean), m->Wf(cb.rstd), m->Wf(cb.a), m->Wf(cb.sg), m->Wf(m->E), m->Wf(m->Ecol), m->Wf(m->Fc), r.key_len, m->W(m->t1), B, T, c, m->s));
        CK(dwconv_bwd_deferred(m, r, 8.0, DWIN_SWISH, m->W(m->t1), nullptr, m->W(cb.z1), cb.dw, -1, m->W(m->t2), c, cb.k, cb.k - 1));
    } else {
        DwBnArgs bn; bn.h = m->W(cb.h2); bn.mean = m->Wf(cb.mean); bn.rstd = m->Wf(cb.rstd); bn.a = m->Wf(cb.a); bn.sg = m->Wf(cb.sg); bn.E = m->Wf(m->E); bn.Fc = m->Wf(m->Fc); bn.e_per_sample = 1;
        CK(dwconv_bn_bwd(m, r, p.bn_bwd == BNB_FUSED, 10.0, DWIN_SWISH, m->W(m->t1), bn, m->W(cb.z1), cb.dw, -1, m->W(m->t2), c, cb.k, cb.k - 1));
    }
    EpiArgs e2; e2.resid = g;
    CK(gemm_dgrad(m, cb.W1, m->W(m->t2), dt, gn, r.M, OP_NONE, no, e2));
    CK(gemm_wgrad(m, cb.W1, x, dt, OP_NONE, no, m->W(m->t2), dt, OP_NONE, no, r.M));
    return 0;
}
