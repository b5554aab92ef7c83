// Shared host-side types of libishara_hip.so: the model handle, its parameter / workspace bookkeeping, the profiled-launch
// macros and what the host units share.  Included by model.hip (handle life cycle and shared plumbing), keras_graph.hip / conv_block.hip /
// keras_hybrid.hip / keras_probe.hip (the Keras get_model family), conformer_r5.hip / squeezeformer_r4.hip (the torch encoder families) and
// api_ops.hip (stand-alone entry points).
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <string>
#include <vector>
#include <map>
#include "kernels.h"
#include "../../include/ishara_hip.h"

#define CK(expr) do { int _r = (expr); if (_r != 0) return _r; } while (0)
// profiled launch: key = kernel family, by = algorithmic bytes, fl = flops of this launch
#define CKP(m, key, by, fl, expr)                                                          \
    do {                                                                                   \
        ProfRec* _pr = nullptr;                                                            \
        if ((m)->prof.on) {                                                                \
            (m)->prof.recs.push_back(ProfRec{key, (m)->prof.get(), (m)->prof.get(), (double)(by), (double)(fl)}); \
            _pr = &(m)->prof.recs.back();                                                  \
            (void)hipEventRecord(_pr->e0, (m)->s);                                         \
        }                                                                                  \
        int _r = (expr);                                                                   \
        if (_pr) (void)hipEventRecord(_pr->e1, (m)->s);                                    \
        if (_r != 0) return _r;                                                            \
    } while (0)

static inline size_t rup(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ------------------------------------------------------------------ model description
struct ParamEntry { std::string name; int ndim; int64_t shape[2]; int64_t offset; bool trainable; };

struct DenseW {           // a Dense / 1x1-conv weight [K,N] (+bias) with its MFMA shadows
    int w = -1, b = -1, K = 0, N = 0;
    size_t wt = 0, wn = 0;    // byte offsets in the workspace
    int ldt = 0, ldn = 0;
};
struct Norm { int gamma = -1, beta = -1; };
struct BNp { int gamma = -1, beta = -1, mm = -1, mv = -1; };

struct Buf { size_t off = 0; };   // byte offset in the workspace

// The launch plan of one Conv1DBlock call (conv_block.hip conv_block_plan: the fields and their conditions)
enum ConvStats { ST_LEN, ST_INFER_PART, ST_TRAIN_PART, ST_SUMS };      // the ECA gate: eca_fwd_len on a masked time mean / _infer / _part on the partial rows / plain on per-sample sums
enum ConvW2Bwd { W2_PSA, W2_FOLDED, W2_SCALED_COPY, W2_PLAIN };        // the project conv's dgrad + wgrad
enum ConvBnBwd { BNB_LEN, BNB_FUSED, BNB_TWO_KERNEL };                 // BatchNorm + depthwise backward: bn_bwd_apply_len + plain / one kernel / bn_bwd_apply + plain
struct ConvPlan {
    bool ok = false;          // false: the depthwise conv refuses the shape
    int prows = 0;            // partial statistic rows per sample of the depthwise forward
    ConvStats stats = ST_SUMS; bool bn_from_part = false, fold = false, prologue = false, psa = false;
    ConvW2Bwd w2_bwd = W2_PLAIN; ConvBnBwd bn_bwd = BNB_TWO_KERNEL;
};
struct ConvBlock {
    DenseW W1, W2; int dw = -1, eca = -1; BNp bn; int k = 0; uint32_t site = 0;
    Buf z1, h2, h4, out, ssum, ssq, mean, rstd, a, bsh, gn, sg, P, Q, rs;
    ConvPlan plan;            // of the last forward: conv_bwd runs what it says
};
struct FFN {
    Norm ln; float eps; DenseW Wa, Wb; uint32_t site_in = 0, site_out = 0; bool has_out_drop = false;
    Buf xn, mean, rstd, za, u, out;
};
struct MHSA {
    Norm ln; float eps; DenseW Wqkv, Wp; float rate = 0.f; uint32_t site_attn = 0, site_out = 0; bool has_out_drop = false;
    Buf xn, mean, rstd, q, k, vt, o, lse, out, maskw;
};
struct SqzConv {
    Norm ln; DenseW Wc1, Wc3; int dw = -1, seW1 = -1, seb1 = -1, seW2 = -1, seb2 = -1; int k = 0, R = 0;
    Buf xn, mean, rstd, zc, zd, hd, u3, gap, hid, se, out;
};
struct ConfConv {
    DenseW Wp1, Wp2; int dw = -1, dwb = -1; BNp bn; Norm ln; int k = 0;
    // Keras defaults (c5:249-309); the torch family overrides them (nn.BatchNorm1d: eps 1e-5, momentum 0.1 on the NEW value, unbiased
    // running variance; nn.LayerNorm eps 1e-5)
    float bn_eps = 1e-3f, bn_keep = 0.99f, ln_eps = 1e-3f; int bn_unbiased = 0;
    // squeezeformer/convolution.py:226-238: Swish between the BatchNorm and the second pointwise conv (sw = swish(bnv)), Dropout on its output
    int swish_after_bn = 0; uint32_t site_out = 0; int has_out_drop = 0; Buf sw;
    Buf g, v, bnv, ssum, ssq, mean, rstd, a, bsh, r, lnmean, lnrstd, out;
};
// ---- torch ConformerEncoder family (conformer/conformer.py:6-87): post-LN sub-modules
struct R5FFN { DenseW W1, W2; Norm ln; uint32_t site_in = 0, site_out = 0; Buf za, u, r, mean, rstd, out;
               float factor = 1.f; };      // r = x + factor * ffn(x)   (squeezeformer half_step_residual: 0.5)
struct R5MHSA { DenseW Wqkv, Wp; Norm ln; uint32_t site_attn = 0; Buf q, k, vt, o, lse, maskw, r, mean, rstd, out; };
struct R5Block { R5FFN ffn1; R5MHSA mha; ConfConv conv; R5FFN ffn2; Norm ln; Buf mean, rstd, out; };
struct Layer {            // one entry of the sequential graph
    enum Kind { CONV, SQZ, CONF } kind;
    int idx;
};
struct SqzBlock { FFN ffn1; MHSA mha; SqzConv conv; FFN ffn2; };
struct ConfBlock { FFN ffn1; MHSA mha; ConfConv conv; FFN ffn2; };

// HIP-event profiler: when enabled every kernel launch site records a (start, stop) event pair
// on the launch stream plus the algorithmic bytes / flops of that launch (bench.py roofline).
struct ProfRec { const char* key; hipEvent_t e0, e1; double bytes, flops; };
struct Profiler {
    bool on = false;
    std::vector<ProfRec> recs;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t get() {
        if (used == pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool.push_back(e); }
        return pool[used++];
    }
};

struct ishara_model {
    ishara_config cfg;
    Profiler prof;
    int dt;                       // activation / MFMA dtype
    int d, T, F, C, H, dh, dtop, Bmax, L;
    std::vector<ParamEntry> entries;
    int64_t n_total = 0, n_train = 0;
    // graph
    DenseW stemW; BNp stem_bn;
    // gradient buckets for an overlapped all-reduce: ranges of the flat gradient, in the order the backward pass completes them
    std::vector<int64_t> bucket_lo, bucket_hi; std::vector<int> bucket_after_layer; std::vector<hipEvent_t> bucket_ev;
    std::vector<size_t> layer_entry_end; size_t stem_entry_end = 0;
    int cls_pad = 0; Buf dlb;          // bf16 model: dlogits also as bf16 [M, cls_pad] (zero padded), 0 = f32 operand path
    int stem_kp = 0; Buf stem_xb;      // bf16 model: input rows packed to bf16 [M, stem_kp] (zero padded), 0 = f32-A GEMM path
    Buf stem_h0, stem_out, stem_ssum, stem_ssq, stem_mean, stem_rstd, stem_a, stem_bsh, pe;
    std::vector<ConvBlock> convs;
    std::vector<SqzBlock> sqz;
    std::vector<ConfBlock> conf;
    std::vector<Layer> layers;
    int family = 0;                    // 0: Keras get_model hybrid; 1: torch ConformerEncoder (conformer_r5.hip)
    std::vector<R5Block> r5; Buf r5_x, t4, fac;          // fac: [Bmax] floats, all = the FFN residual factor (epilogue row scale)
    struct R4State* r4 = nullptr;                          // torch Squeezeformer family (squeezeformer_r4.hip)
    DenseW topW, clsW; uint32_t head_site = 0; Buf head_hh;
    uint32_t nsites = 0;
    std::vector<DenseW*> denses;
    // temps
    RedSink red; Buf red_arena; size_t red_cap = 0, red_off = 0; bool red_on = false;      // deferred column sums of LayerNorm / depthwise-conv parameter gradients (model.hip red_scratch)
    TnDefer tn_defer; Buf slab2[2]; bool tn_defer_on = false;      // deferred wgrad slab sums (gemm_tn.hip): two alternating slab buffers
    Buf gA, gB, t1, t2, t3, S1, S2, E, Fc, Ecol, ecap, dse, dgapT, slab, ctcws, dlogits, nllb, delta;
    Buf psaG, psaR; bool psa_on = false;   // TnPsa outputs: G [B, d], Rpart [B][d / 64][2d]
    size_t shadow_begin = 0, shadow_end = 0;
    size_t shadow_tab_off = 0;             // device descriptor table of the batched shadow build, inside the workspace (no
                                           // hipMalloc/hipFree of our own: a hipFree from a garbage-collected model would break a
                                           // stream capture in progress elsewhere in the process)
    std::vector<ShadowDesc> shadow_tab_host;
    int shadow_ntab = 0, shadow_tiles = 0;
    bool shadow_ready = false;
    size_t ws_need = 0;
    // bound
    float* params = nullptr; float* grads = nullptr; float* om = nullptr; float* ov = nullptr; float* oslow = nullptr;
    char* ws = nullptr; int64_t ws_bytes = 0;
    std::vector<float> pe_host;
    // run state
    int lastB = 0; int last_training = 0; uint32_t last_seed = 0; const float* last_x = nullptr;
    int last_masked = 0;            // the last ishara_encoder_forward(_ex) was given an attention mask, the last ishara_forward(_ex) frame lengths (the arrays themselves are the caller's: no pointer is kept)
    int probe_masked = 0;           // the same bit for the module probe's last training forward
    int opt_iter = 0;
    int probe_mod = -1, probe_B = 0; uint32_t probe_seed = 0;      // module probe (ishara_debug_module_*): the last training forward of a single module
    hipStream_t s = nullptr;

    // ---- build helpers
    int addp(const std::string& name, int64_t r, int64_t c, bool trainable) {
        ParamEntry e; e.name = name; e.ndim = c > 0 ? 2 : 1; e.shape[0] = r; e.shape[1] = c > 0 ? c : 0; e.offset = -1; e.trainable = trainable;
        entries.push_back(e);
        return (int)entries.size() - 1;
    }
    size_t cur = 0;
    // ISHARA_WS_GUARD=1 (read at ishara_create): every workspace buffer is followed by a 256-byte guard zone that ishara_bind fills
    // with a pattern and ishara_workspace_guard_check verifies — an out-of-bounds write of any kernel into a neighbouring buffer
    // shows up as a named offset instead of as silent corruption (tests/test_tflite_gpu.py, tests/test_model_gpu.py)
    bool guard = false; std::vector<size_t> guard_offs; std::vector<std::pair<size_t, size_t>> allocs;
    Buf alloc(size_t bytes) {
        Buf b; b.off = cur; cur = rup(cur + bytes, 256);
        allocs.push_back({b.off, bytes});
        if (guard) { guard_offs.push_back(cur); cur += 256; }
        return b;
    }
    Buf act(int cols) { return alloc((size_t)Bmax * T * cols * dt_size(dt)); }
    Buf f32(size_t n) { return alloc(n * sizeof(float)); }
    DenseW dense_named(const std::string& wname, const std::string& bname, int K, int N) {      // empty bname: no bias
        DenseW w; w.K = K; w.N = N;
        w.w = addp(wname, K, N, true);
        if (!bname.empty()) w.b = addp(bname, N, 0, true);
        return w;
    }
    DenseW dense(const std::string& name, int K, int N, bool bias) { return dense_named(name + "/kernel", bias ? name + "/bias" : "", K, N); }      // Keras names
    Norm norm(const std::string& name, int c) { Norm n; n.gamma = addp(name + "/gamma", c, 0, true); n.beta = addp(name + "/beta", c, 0, true); return n; }
    Norm norm_named(const std::string& prefix, int c) { Norm n; n.gamma = addp(prefix + ".weight", c, 0, true); n.beta = addp(prefix + ".bias", c, 0, true); return n; }      // torch state_dict names
    BNp bnp(const std::string& name, int c) {
        BNp b; b.gamma = addp(name + "/gamma", c, 0, true); b.beta = addp(name + "/beta", c, 0, true);
        b.mm = addp(name + "/moving_mean", c, 0, false); b.mv = addp(name + "/moving_variance", c, 0, false);
        return b;
    }
    float* P(int idx) const { return params + entries[idx].offset; }
    float* G(int idx) const { return grads + entries[idx].offset; }
    template <typename TT = void> TT* W(Buf b) const { return reinterpret_cast<TT*>(ws + b.off); }
    float* Wf(Buf b) const { return reinterpret_cast<float*>(ws + b.off); }
};


// ------------------------------------------------------------------ shared helpers (model.hip unless noted)
// attn_bias / key_len: the caller's attention mask arrays of this one call (ishara_encoder_forward_ex / _backward_ex), nullptr otherwise;
// in the Keras hybrid family key_len is the per-clip frame count of ishara_forward_ex / ishara_loss_backward_ex (keras_hybrid.hip)
struct Run { int B, M, training; uint32_t seed; const float* attn_bias = nullptr; const int* key_len = nullptr; };
static inline DropSpec dspec(const Run& r, uint32_t site, float rate) { return make_drop(r.seed, site, rate, r.training != 0); }
static inline DropSpec dspec_attn(const Run& r, uint32_t site, float rate) { return make_drop_attn(r.seed, site, rate, r.training != 0); }   // attention probabilities: common.h rng_quad
void finish_param_layout(ishara_model* m);      // after the last addp: offsets, n_train, n_total
static inline int shadow_ld(int dt, int cols, int min_ld = 0) {      // row stride of a weight shadow: whole K tiles of the MFMA kernels (zero padded)
    const int ld = (int)rup(cols, dt_is16(dt) ? 64 : 32);
    return ld < min_ld ? min_ld : ld;
}
void plan_shadow(ishara_model* m, DenseW& w, int min_ldt = 0, int min_ldn = 0);
void plan_confconv(ishara_model* m, ConfConv& c, size_t rows, int B, int d);
void plan_post_ln_ffn(ishara_model* m, R5FFN& f, size_t rows, int d, int de);
size_t wgrad_slab_floats(const ishara_model* m, size_t M, int min_K = 0);
size_t slab_floats(const ishara_model* m, size_t M, int B, int T, int maxw, int min_K = 0);
// profiled GEMM launches over a planned Dense weight: forward C = epi(A W), dgrad dX = epi(dY W^T), wgrad dW += A^T dY (+ bias grad)
int gemm_fwd(ishara_model* m, const DenseW& w, const void* A, int dtA, void* Cc, int dtC, int M, int aop, const OpArgs& oa, EpiArgs ea);
int gemm_dgrad(ishara_model* m, const DenseW& w, const void* dY, int dtA, void* dX, int M, int aop, const OpArgs& oa, const EpiArgs& ea);
int gemm_wgrad(ishara_model* m, const DenseW& w, const void* A, int dtA, int aop, const OpArgs& oa, const void* dY, int dtB, int bop, const OpArgs& ob, int M, int ka_valid = 0, int nb_valid = 0,
               const float* bias_rowscale = nullptr, int bias_T = 0, const TnPsa* psa = nullptr);
int wgrad_flush(ishara_model* m);
int red_flush(ishara_model* m);
int layernorm_bwd_deferred(ishara_model* m, const Run& r, const void* dy, const void* x, Buf mean, Buf rstd, const Norm& ln, const void* resid, void* dx);
int dwconv_bwd_deferred(ishara_model* m, const Run& r, double by_factor, int inop, const void* dy, const DwBnArgs* bn, const void* x, int dw, int dwb, void* dx, int C, int k, int padl);
const void* grad_through_dropout(ishara_model* m, const Run& r, uint32_t site, float rate, const void* g, void* tmp, int T, int cols, int* rc);
// Keras get_model hybrid family: graph and workspace plan (keras_graph.hip)
void keras_build_graph(ishara_model* m);
void keras_plan_workspace(ishara_model* m);
// its Conv1DBlock (conv_block.hip): the plan, the module, the two launch pairs it shares with the Conformer conv module, the fusion switches
bool infer_fusion_on();       // ISHARA_NO_INFER_FUSION unset (read at every call)
bool stats_fusion_on();       // ISHARA_NO_STATS_FUSION unset (read once per process)
ConvPlan conv_block_plan(int dt, bool training, int B, int T, int d, int k, int ldt, int ldn, bool drop_path, bool lengths, bool psa_on);
const char* conv_block_route_name(const ConvPlan& p, bool training);
int conv_fwd(ishara_model* m, ConvBlock& cb, const Run& r, const void* x);
int conv_bwd(ishara_model* m, ConvBlock& cb, const Run& r, const void* x, const void* g, void* gn);
struct DwBnFwd { BNp bn; float eps, keep, var_corr; Buf ssum, ssq, mean, rstd, a, bsh; };      // a BatchNorm behind a depthwise conv: parameters, constants, buffers
int dwconv_stat_rows(int dt, int B, int T, int C, int k);      // partial statistic rows per sample of a depthwise forward with statistics
int dwconv_bn_fwd(ishara_model* m, const Run& r, int inop, const void* x, int dw, int dwb, void* y, int C, int k, int padl, const DwBnFwd& s, bool with_sums, int prows, bool finalize);
bool dwconv_bwd_fused_bn(int dt, int C, int k, int padl);
int dwconv_bn_bwd(ishara_model* m, const Run& r, bool fused, double by_fused, int inop, void* dy, const DwBnArgs& bn, const void* x, int dw, int dwb, void* dx, int C, int k, int padl);
// the other modules, stem and head (keras_hybrid.hip; the module probe in keras_probe.hip runs them one at a time); confconv_* also serve the torch
// families, ln_as_prologue / classifier_fwd the operator entry points
int ffn_fwd(ishara_model* m, FFN& f, const Run& r, const void* x);
int ffn_bwd(ishara_model* m, FFN& f, const Run& r, const void* x, const void* g, void* gn);
int mhsa_fwd(ishara_model* m, MHSA& a, const Run& r, const void* x);
int mhsa_bwd(ishara_model* m, MHSA& a, const Run& r, const void* x, const void* g, void* gn);
int sqzconv_fwd(ishara_model* m, SqzConv& c, const Run& r, const void* x);
int sqzconv_bwd(ishara_model* m, SqzConv& c, const Run& r, const void* x, const void* g, void* gn);
int stem_fwd(ishara_model* m, const Run& r, const float* x);
int stem_bwd(ishara_model* m, const Run& r, const void* g);
int head_fwd(ishara_model* m, const Run& r, const void* h, float* logits);
int head_bwd(ishara_model* m, const Run& r, const void* hin, void* g);
bool frame_len_ok(const ishara_model* m, const char* fn, const int32_t* frame_len);
bool frame_len_agrees(const char* fn, bool fwd_had, const int32_t* frame_len);
bool ln_as_prologue(int dt, int M, int N, int K, int ldt, const float* gamma, const float* beta, float eps, float* mean, float* rstd, void* xn, EpiArgs& ea);
enum { CLS_AUTO = 0, CLS_AS = 1, CLS_NARROW = 2, CLS_GEMM = 3 };      // routes of classifier_fwd
int cls_route_auto(int dt, int M, int K, int C);
int classifier_fwd(ishara_model* m, int route, int dt, const void* A, const void* Wt, int ldt, const float* bias, float* logits, int M, int K, int C, hipStream_t s);
int confconv_fwd(ishara_model* m, ConfConv& c, const Run& r, const void* x);
int confconv_bwd(ishara_model* m, ConfConv& c, const Run& r, const void* x, const void* g, void* gn);
int r5_ffn_fwd(ishara_model* m, R5FFN& f, const Run& r, const void* x);
int r5_ffn_bwd(ishara_model* m, R5FFN& f, const Run& r, const void* x, const void* g, void* gn);
int r5_ln_fwd(ishara_model* m, const Run& r, const void* x, const Norm& n, void* y, Buf mean, Buf rstd);
int r5_ln_bwd(ishara_model* m, const Run& r, const void* g, const void* x, const Norm& n, Buf mean, Buf rstd, void* dx);
int r5_from_f32(int dt, const float* x, void* y, size_t n, hipStream_t s);
int r5_to_f32(int dt, const void* x, float* y, size_t n, hipStream_t s);
// torch ConformerEncoder family (conformer_r5.hip)
int r5_validate(const ishara_config& c);
void r5_build_graph(ishara_model* m);
void r5_plan_workspace(ishara_model* m);
// torch Squeezeformer family (squeezeformer_r4.hip; its kernels: r4_subsample.hip, relattn_len.hip, relattn_mfma.hip)
int r4_validate(const ishara_config& c);
void r4_build_graph(ishara_model* m);
void r4_plan_workspace(ishara_model* m);
int r4_bind(ishara_model* m);
void r4_destroy(ishara_model* m);
int r4_output_frames(const ishara_model* m);
// input_len: device int32 [B], input frames per clip (ishara_encoder_forward_lengths / _backward_lengths); nullptr: the unmasked pass
int r4_forward(ishara_model* m, const float* x, int32_t B, float* y, int32_t training, uint32_t seed, hipStream_t st, const int32_t* input_len = nullptr);
int r4_backward(ishara_model* m, const float* dy, int32_t B, float* dx, hipStream_t st, const int32_t* input_len = nullptr);
// its launch code, shared with the operator entry points (api_ops.hip ishara_op_relattn_* / ishara_relattn_len_* / ishara_op_r4_*)
// relative-position attention (relattn_len.hip, relattn_mfma.hip).  The head dims the kernels are instantiated for, stated once
#define RELATTN_HEAD_DIMS "8, 16, 32, 64"
inline bool relattn_head_dim_ok(int dh) { return dh == 8 || dh == 16 || dh == 32 || dh == 64; }
// which kernels a call runs is stated once, by relattn_route; key_len nullptr (masked = false) is the call without lengths: every key
enum { RELATTN_REFUSED = 0, RELATTN_LANE = 1, RELATTN_MFMA_LEN = 3 };      // LANE: the fp32 lane kernels; MFMA_LEN: MFMA forward (relattn_mfma.hip), lane backward
struct RelAttnRoute { int kind = RELATTN_REFUSED; const char* why = ""; };
RelAttnRoute relattn_route(int dt, int T, int dh, bool masked);
const char* relattn_kernel_name(const RelAttnRoute& r, bool backward);
// force_lane: the lane forward where the route would choose the MFMA one (the backward has one route)
int launch_relattn_len_fwd(int dt, const void* q, const void* k, const void* v, const float* posp, const float* u, const float* vb, void* o, float* lse,
                           const int* key_len, bool force_lane, int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s);
int launch_relattn_len_bwd(int dt, const void* q, const void* k, const void* v, const float* posp, const float* u, const float* vb, const void* o, const void* dO,
                           const float* lse, float* delta, void* dq, void* dk, void* dv, float* du, float* dvb, float* dposp,
                           const int* key_len, int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s);
int launch_relattn_len_fwd_mfma(const void* q, const void* k, const void* v, const float* posp, const float* u, const float* vb, void* o, float* lse,
                                const int* key_len, int B, int H, int T, int dh, float scale, DropSpec drop, hipStream_t s);
// subsampling, time reduction, row maps and stage lengths (r4_subsample.hip)
struct R4Dims { int T1, F1, T2, F2, T3, Fr, Kp; };      // frames / features after each 3x3 stride-2 convolution, the time-reduction conv's width and its padded K
R4Dims r4_dims(int T0, int F, int d);
enum { R4_ROWS_RECOVER = 0, R4_ROWS_CROP = 1, R4_ROWS_RECOVER_BWD = 2, R4_ROWS_CROP_BWD = 3, R4_ROWS_ADD = 4 };      // r4_rows_mode_launch's modes; the integers are the ABI of ishara_op_r4_rows
int r4_stage_len_launch(const int* L, int* out, int B, int T0, int T2, int T3, int Trec, hipStream_t s);      // int32 [3][B]: keys at T2, T3, Trec
int r4_subsample_fwd_launch(int dt, const float* x, const float* w1, const float* b1, const float* w2, const float* b2, float* y1, void* sub,
                            int B, int T0, int F, int d, int T1, int F1, int T2, int F2, hipStream_t s);
int r4_subsample_bwd_launch(int dt, const void* dsub, const void* sub, const float* y1, const float* x, const float* w1, const float* w2, float* dz1,
                            float* dw1, float* db1, float* dw2, float* db2, float* dx, int B, int T0, int F, int d, int T1, int F1, int T2, int F2, hipStream_t s);
int r4_tred_fwd_launch(int dt, const void* h, const float* w, const float* b, float* pre, void* out, int B, int Tin, int d, int Tr, int Fr, int Kp, hipStream_t s);
int r4_tred_wgrad_launch(int dt, const void* trout, const void* g, float* dwred, float* dW, float* db, float* slab, int M, int Fr, int Kp, int d, hipStream_t s);
int r4_tred_bwd_launch(int dt, const void* dout, const float* pre, const void* h, const float* w, const void* extra, float* dw, float* db, void* dh,
                       int B, int Tin, int d, int Tr, int Fr, int Kp, hipStream_t s);
int r4_rows_mode_launch(int dt, int mode, const void* src, const void* a, void* dst, int B, int Tdst, int Tsrc, int d, hipStream_t s);
int r4_fill_f32_launch(float* p, size_t n, float v, hipStream_t s);
