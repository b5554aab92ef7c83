// Handle-free entry points of the forward / dgrad tile GEMMs (gemm_nt.hip: gemm_nt_t_kernel, gemm_nt_glds_kernel, gemm_nt_kernel):
// ishara_op_gemm_nt runs ONE launch_gemm_nt call with the arguments the models pass — three dtypes, an operand transform, the whole epilogue —
// on a weight shadow the caller built, so nothing but the GEMM kernel is in the launch sequence (no memset, no make_shadow_kernel);
// ishara_debug_gemm_nt_route reports the route and the profiler key of a call from gemm_nt_route, the function the launcher launches from.
// The A-stationary family's entries (ishara_op_gemm_as, ishara_debug_gemm_as_plan) and its own padding contract are at the end of the file.
//
// The padding contract of Bt [bt_rows][ldb] (dtM), which every tile kernel relies on and the entry cannot see:
//   rows n in [N, roundup(N, 128)) are READ by every kernel (it computes the whole 128-column tile) and their products are discarded by the
//     column guards of the epilogue: any finite or non-finite value may stand there;
//   columns k in [K, ldb) of every row must be ZERO: gemm_nt_kernel multiplies them with its zero-filled A tail up to roundup(K, 64 / 32)
//     (0 * NaN would poison the sum); the LDS-DMA kernels take only K % K-tile == 0 and never read them.
// c1 / c0 of OP_COLAFFINE are read up to roundup(K, 64 / 32) floats (the transform runs on the zero-filled tail before it is cleared again).
#include <string>
#include "kernels.h"

typedef ishara_gemm_nt_call NtCall;

static const char* nt_route_text(NtRoute r) {
    switch (r) {
        case NT_REFUSED: return "NT_REFUSED";
        case NT_AS_F16: return "NT_AS_F16";
        case NT_BIG: return "NT_BIG";
        case NT_CS: return "NT_CS";
        case NT_AS: return "NT_AS";
        case NT_TILE_T: return "NT_TILE_T";
        case NT_GLDS: return "NT_GLDS";
        case NT_REG: return "NT_REG";
    }
    return "NT_REFUSED";
}
static bool nt_rate_ok(float r) { return r >= 0.f && r < 1.f; }      // (false for NaN)
static EpiArgs nt_call_epi(const NtCall& c) {
    EpiArgs ea;
    ea.bias = c.bias; ea.addtab = c.addtab; ea.tab_period = c.tab_period; ea.pre_out = c.pre_out; ea.act = c.act;
    ea.drop = make_drop(c.drop_seed, c.drop_site, c.drop_rate, true);
    ea.rowscale = c.rowscale; ea.T = c.T; ea.rowscale_bias = c.rowscale_bias; ea.dact = c.dact; ea.aux = c.aux; ea.resid = c.resid;
    ea.mode = c.mode; ea.q = c.q; ea.k = c.k; ea.vt = c.vt; ea.H = c.H; ea.dh = c.dh; ea.head_major = c.head_major;
    return ea;
}
static OpArgs nt_call_op(const NtCall& c) {
    OpArgs oa;
    oa.c1 = c.c1; oa.c0 = c.c0;
    oa.drop = make_drop(c.op_seed, c.op_site, c.op_rate, true);
    return oa;
}
// the launcher's own refusals (launch_gemm_nt returns -1 with its message before any HIP call): a bad shape, A rows off 16 bytes, a QKV split
// off multiples of 8, a call gemm_nt_route refuses
static bool nt_launcher_refuses(const NtCall& c, const EpiArgs& ea, NtRoute* route) {
    *route = NT_REFUSED;
    if (c.M <= 0 || c.N <= 0 || c.K <= 0) return true;
    if ((dt_is16(c.dtA) && c.K % 8 != 0) || (c.dtA == DT_F32 && c.K % 4 != 0) || ((uintptr_t)c.A) % 16 != 0) return true;
    if (ea.mode == EPI_QKV && (ea.T % 8 != 0 || c.N % 8 != 0 || ea.dh % 8 != 0)) return true;
    *route = gemm_nt_route(c.dtA, c.dtM, c.dtC, c.op, c.A, c.M, c.N, c.K, c.ldb, ea);
    return *route == NT_REFUSED;
}
static int nt_rup(int x, int m) { return (x + m - 1) / m * m; }

// everything about the call that a launch would fault or fail on, before any HIP call: the entry's own checks, each naming its field, then the
// launcher's (its message behind the entry's name).  0: *route is one of NT_TILE_T / NT_GLDS / NT_REG and the call may be launched
static int nt_fields_refused(const char* me, const NtCall& c);
static int nt_call_refused(const char* me, const NtCall& c, NtRoute* route) {
    *route = NT_REFUSED;
    if (nt_fields_refused(me, c)) return -1;
    const EpiArgs ea = nt_call_epi(c);
    if (nt_launcher_refuses(c, ea, route)) {          // the launcher's message, behind the entry's name (it refuses before any HIP call)
        const OpArgs oa = nt_call_op(c);
        const int rc = launch_gemm_nt(c.dtA, c.dtM, c.dtC, c.op, c.A, c.Bt, c.C, c.M, c.N, c.K, c.ldb, oa, ea, nullptr);
        const char* le = ishara_last_error();
        const std::string why = (rc != 0 && le) ? le : "internal error: the launcher took a call the entry expected it to refuse";
        ishara_set_error("%s: %s", me, why.c_str());
        *route = NT_REFUSED;
        return -1;
    }
    if (*route != NT_TILE_T && *route != NT_GLDS && *route != NT_REG) {
        ishara_set_error("%s: route %s: only the tile kernels of gemm_nt.hip are served (NT_TILE_T, NT_GLDS, NT_REG; ishara_debug_force_regstage 8192 / 8 / 1 selects them)",
                         me, nt_route_text(*route));
        *route = NT_REFUSED;
        return -1;
    }
    // the weight shadow: whole 128-row column tiles, rows of whole K tiles of the route (LDS-DMA kernels 32 bf16 / 16 f32, register-staged 64 / 32)
    const int es = (int)dt_size(c.dtM);
    const int bk = (*route == NT_REG ? 2 : 1) * (dt_is16(c.dtM) ? 32 : 16);
    if (c.bt_rows < nt_rup(c.N, 128)) { ishara_set_error("%s: bt_rows=%d < roundup(N=%d, 128): every kernel reads whole 128-row tiles of Bt", me, c.bt_rows, c.N); *route = NT_REFUSED; return -1; }
    if (c.ldb < nt_rup(c.K, bk) || (c.ldb * es) % 16 != 0) {
        ishara_set_error("%s: ldb=%d: needs >= roundup(K=%d, %d) and rows of whole 16-byte pieces (%s)", me, c.ldb, c.K, bk, nt_route_text(*route)); *route = NT_REFUSED; return -1;
    }
    // outputs and side operands, each to its widest access: the accumulator-layout epilogue of the 128 x 128 tile kernel moves 4 elements, the
    // row-chunk epilogue of the other two 8
    const uintptr_t wide = (*route == NT_TILE_T && dt_is16(c.dtC)) ? 8 : 16;
    const void* tc[7] = {c.C, c.pre_out, c.aux, c.resid, c.q, c.k, c.vt};
    const char* tcn[7] = {"C", "pre_out", "aux", "resid", "q", "k", "vt"};
    for (int k = 0; k < 7; ++k)
        if ((uintptr_t)tc[k] % wide != 0) { ishara_set_error("%s: misaligned %s (%d-byte aligned on %s)", me, tcn[k], (int)wide, nt_route_text(*route)); *route = NT_REFUSED; return -1; }
    if ((uintptr_t)c.addtab % (*route == NT_TILE_T ? 16 : 4) != 0) { ishara_set_error("%s: misaligned addtab (%d-byte aligned on %s)", me, *route == NT_TILE_T ? 16 : 4, nt_route_text(*route)); *route = NT_REFUSED; return -1; }
    const void* f4[4] = {c.bias, c.rowscale, c.c1, c.c0};
    const char* f4n[4] = {"bias", "rowscale", "c1", "c0"};
    for (int k = 0; k < 4; ++k)
        if ((uintptr_t)f4[k] % 4 != 0) { ishara_set_error("%s: misaligned %s (4-byte aligned)", me, f4n[k]); *route = NT_REFUSED; return -1; }
    return 0;
}

// the checks of the call's own fields that both entries make (ishara_op_gemm_nt, ishara_op_gemm_as), each naming its field
static int nt_fields_refused(const char* me, const NtCall& c) {
    const int dts[3] = {c.dtA, c.dtM, c.dtC};
    const char* names[3] = {"dtA", "dtM", "dtC"};
    for (int k = 0; k < 3; ++k)
        if (dts[k] != DT_F32 && dts[k] != DT_BF16 && dts[k] != DT_F16) {
            ishara_set_error("%s: unknown dtype %s=%d (ISHARA_F32 = 0, ISHARA_BF16 = 1, ISHARA_F16 = 2)", me, names[k], dts[k]); return -1;
        }
    if (c.op < OP_NONE || c.op > OP_DROPMASK) { ishara_set_error("%s: unknown op=%d (0 none, 1 swish, 2 column affine, 4 dropout mask)", me, c.op); return -1; }
    if (c.op == OP_ROWSCALE) { ishara_set_error("%s: op=3 (OP_ROWSCALE) is not carried: no forward or dgrad GEMM of the models passes it", me); return -1; }
    if (c.op == OP_COLAFFINE && (!c.c1 || !c.c0)) { ishara_set_error("%s: op=2 (OP_COLAFFINE) without c1 / c0", me); return -1; }
    if (c.act < ACT_NONE || c.act > ACT_RELU) { ishara_set_error("%s: unknown act=%d", me, c.act); return -1; }
    if (c.dact < DACT_NONE || c.dact > DACT_POS) { ishara_set_error("%s: unknown dact=%d", me, c.dact); return -1; }
    if (c.mode != EPI_STD && c.mode != EPI_QKV) { ishara_set_error("%s: unknown mode=%d (0 standard, 1 QKV split)", me, c.mode); return -1; }
    if (c.head_major != 0 && c.head_major != 1) { ishara_set_error("%s: head_major=%d (0 or 1)", me, c.head_major); return -1; }
    if (c.rowscale_bias != 0 && c.rowscale_bias != 1) { ishara_set_error("%s: rowscale_bias=%d (0 or 1)", me, c.rowscale_bias); return -1; }
    if (!nt_rate_ok(c.op_rate)) { ishara_set_error("%s: op_rate %g outside [0, 1)", me, (double)c.op_rate); return -1; }
    if (!nt_rate_ok(c.drop_rate)) { ishara_set_error("%s: drop_rate %g outside [0, 1)", me, (double)c.drop_rate); return -1; }
    if (!c.A) { ishara_set_error("%s: null A", me); return -1; }
    if (!c.Bt) { ishara_set_error("%s: null Bt", me); return -1; }
    if (!c.C && c.mode != EPI_QKV) { ishara_set_error("%s: null C (only a QKV split writes no C)", me); return -1; }
    if ((uintptr_t)c.Bt % 16 != 0) { ishara_set_error("%s: misaligned Bt (16-byte aligned)", me); return -1; }
    if (c.addtab && c.tab_period < 1) { ishara_set_error("%s: addtab with tab_period=%d < 1", me, c.tab_period); return -1; }
    if (c.rowscale && c.T < 1) { ishara_set_error("%s: rowscale with T=%d < 1", me, c.T); return -1; }
    if (c.dact != DACT_NONE && !c.aux) { ishara_set_error("%s: dact=%d without aux", me, c.dact); return -1; }
    if (c.mode == EPI_QKV) {
        if (!c.q || !c.k || !c.vt) { ishara_set_error("%s: QKV split without all of q, k, vt", me); return -1; }
        if (c.T < 1 || c.H < 1 || c.dh < 1) { ishara_set_error("%s: QKV split with T=%d H=%d dh=%d (each >= 1)", me, c.T, c.H, c.dh); return -1; }
        if (c.M % c.T != 0) { ishara_set_error("%s: QKV split with M=%d not a multiple of T=%d", me, c.M, c.T); return -1; }
        if ((int64_t)c.N != 3 * (int64_t)c.H * c.dh) { ishara_set_error("%s: QKV split with N=%d != 3 * H * dh = 3 * %d * %d", me, c.N, c.H, c.dh); return -1; }
    }
    return 0;
}

extern "C" int ishara_op_gemm_nt(const ishara_gemm_nt_call* call, ishara_stream st) {
    const char* me = "ishara_op_gemm_nt";
    if (!call) { ishara_set_error("%s: null call", me); return -1; }
    NtRoute route;
    if (nt_call_refused(me, *call, &route)) return -1;
    const NtCall& c = *call;
    const EpiArgs ea = nt_call_epi(c);
    const OpArgs oa = nt_call_op(c);
    return launch_gemm_nt(c.dtA, c.dtM, c.dtC, c.op, c.A, c.Bt, c.C, c.M, c.N, c.K, c.ldb, oa, ea, (hipStream_t)st);
}

extern "C" int ishara_debug_gemm_nt_route(const ishara_gemm_nt_call* call, const char** route, const char** kernel) {
    const char* me = "ishara_debug_gemm_nt_route";
    if (!call || !route || !kernel) { ishara_set_error("%s: null argument", me); return -1; }
    *route = "NT_REFUSED"; *kernel = "";
    NtRoute r;
    if (nt_call_refused(me, *call, &r)) return 0;      // the reason is in ishara_last_error
    const EpiArgs ea = nt_call_epi(*call);
    *route = nt_route_text(r);
    *kernel = gemm_nt_kernel_name(call->dtA, call->dtM, call->dtC, call->op, call->A, call->M, call->N, call->K, call->ldb, ea);
    return 0;
}

// ---- the A-stationary family (gemm_as.hip, gemm_as_f16.hip): ishara_op_gemm_as runs ONE launch_gemm_nt call that lands on NT_AS / NT_AS_F16, with
// the fields of EpiArgs only that family reads (ishara_gemm_as_ext); ishara_debug_gemm_as_plan reports gemm_nt_as_plan, which run_as launches from.
//
// The padding contract of this family's Bt [bt_rows][ldb] (16-bit operand type): a workgroup's LDS-DMA reads the rows [nbase, nbase + nsteps * 32)
// of its column split, N rows in all, and of each row the 16-byte pieces 0 .. K / 8 - 1: rows n >= N are NEVER read (bt_rows = N is enough) and
// columns k >= K are NEVER read (any value may stand in [K, ldb)); ldb % 64 keeps every row's pieces 16-byte aligned for the DMA.
typedef ishara_gemm_as_ext AsExt;
static EpiArgs as_call_epi(const NtCall& c, const AsExt& x) {
    EpiArgs ea = nt_call_epi(c);
    ea.ln_gamma = x.ln_gamma; ea.ln_beta = x.ln_beta; ea.ln_eps = x.ln_eps; ea.ln_mean = x.ln_mean; ea.ln_rstd = x.ln_rstd;
    ea.pa_P = x.pa_P; ea.pa_Q = x.pa_Q; ea.pro_out = x.pro_out; ea.ldc = x.ldc; ea.n_valid = x.n_valid; ea.as_flags = x.as_flags;
    return ea;
}
// 0: the call lands on NT_AS / NT_AS_F16 (*route), *plan is what run_as launches from, and nothing in it would fault
static int as_call_refused(const char* me, const NtCall& c, const AsExt& x, NtRoute* route, AsPlan* plan) {
#define AS_REFUSE(...) do { ishara_set_error(__VA_ARGS__); *route = NT_REFUSED; return -1; } while (0)
    *route = NT_REFUSED;
    if (nt_fields_refused(me, c)) return -1;
    // the ext's own fields
    if (x.as_flags < -1 || x.as_flags > 511) AS_REFUSE("%s: as_flags=%d (-1: the library default, else bits 0 .. 8)", me, x.as_flags);
    if (x.ln_gamma && x.pa_P) AS_REFUSE("%s: ln_gamma and pa_P: one operand prologue at most", me);
    if ((x.ln_gamma != nullptr) != (x.ln_beta != nullptr)) AS_REFUSE("%s: ln_gamma and ln_beta: both or neither", me);
    if ((x.pa_P != nullptr) != (x.pa_Q != nullptr)) AS_REFUSE("%s: pa_P and pa_Q: both or neither", me);
    if ((x.ln_mean != nullptr) != (x.ln_rstd != nullptr)) AS_REFUSE("%s: ln_mean and ln_rstd: both or neither", me);
    if (x.ln_mean && !x.ln_gamma) AS_REFUSE("%s: ln_mean / ln_rstd without ln_gamma", me);
    if (x.pro_out && !x.ln_gamma && !x.pa_P) AS_REFUSE("%s: pro_out without a prologue (ln_gamma or pa_P)", me);
    if (x.ln_gamma && !(x.ln_eps >= 0.f && x.ln_eps < 1e30f)) AS_REFUSE("%s: ln_eps %g (finite, >= 0)", me, (double)x.ln_eps);
    if (x.pa_P && c.T < 1) AS_REFUSE("%s: pa_P with T=%d < 1", me, c.T);
    const int esC = (int)dt_size(c.dtC), group = 16 / esC;
    if (((int64_t)x.ldc * esC) % 16 != 0) AS_REFUSE("%s: ldc=%d: rows of C must be whole 16-byte pieces apart", me, x.ldc);
    if (x.n_valid < 0 || x.n_valid > c.N) AS_REFUSE("%s: n_valid=%d outside [0, N=%d]", me, x.n_valid, c.N);
    if (x.ldc < 0 || (x.ldc && x.ldc < (x.n_valid ? x.n_valid : c.N))) AS_REFUSE("%s: ldc=%d (0, or at least the %d columns a row stores)", me, x.ldc, x.n_valid ? x.n_valid : c.N);
    if (x.n_valid % group != 0) AS_REFUSE("%s: n_valid=%d is not a multiple of the 16-byte store group (%d columns of this dtC): the group that holds it would be stored whole", me, x.n_valid, group);
    if ((x.ldc || x.n_valid) && (c.resid || c.aux || c.mode == EPI_QKV))
        AS_REFUSE("%s: ldc=%d / n_valid=%d with %s: the narrow output has no residual, act' operand or QKV split", me, x.ldc, x.n_valid, c.resid ? "resid" : (c.aux ? "aux" : "QKV"));
    // the weight shadow (before the route: a stride the LDS-DMA cannot take would send the call to another kernel)
    if (c.bt_rows < c.N) AS_REFUSE("%s: bt_rows=%d < N=%d", me, c.bt_rows, c.N);
    if (c.ldb < c.K || c.ldb % 64 != 0) AS_REFUSE("%s: ldb=%d: needs >= K=%d and a multiple of 64", me, c.ldb, c.K);
    const EpiArgs ea = as_call_epi(c, x);
    // a prologue the kernels are not compiled for (run_as would find it at launch, or the fp16 route would ignore it)
    const bool as_shape = dt_is16(c.dtM) && c.dtA == c.dtM && (c.K == 128 || c.K == 256 || c.K == 512 || c.K == 1024) && c.N > 0 && c.N % 32 == 0 && c.M > 0;
    if (as_shape && (x.ln_gamma || x.pa_P)) {
        if (!gemm_nt_as_plan(c.dtM, c.dtC, c.M, c.N, c.K, ea, plan))
            AS_REFUSE("%s: %s prologue with dtC=%d, K=%d and the epilogue mask %d: run_as has no instantiation for it (operand-type C, K >= 256; LayerNorm: mask 0, 36, 44, 64; affine: 1, 17)",
                      me, x.ln_gamma ? "ln_gamma: LayerNorm" : "pa_P: affine", c.dtC, c.K, gemm_nt_as_mask(ea));
        if (x.pa_P && c.T % plan->rows != 0) AS_REFUSE("%s: pa_P with T=%d not a multiple of the %d rows per workgroup: a workgroup's rows must lie inside one sample", me, c.T, plan->rows);
    }
    if (nt_launcher_refuses(c, ea, route)) {          // the launcher's message, behind the entry's name (it refuses before any HIP call)
        const OpArgs oa = nt_call_op(c);
        const int rc = launch_gemm_nt(c.dtA, c.dtM, c.dtC, c.op, c.A, c.Bt, c.C, c.M, c.N, c.K, c.ldb, oa, ea, nullptr);
        const char* le = ishara_last_error();
        const std::string why = (rc != 0 && le) ? le : "internal error: the launcher took a call the entry expected it to refuse";
        AS_REFUSE("%s: %s", me, why.c_str());
    }
    if (*route != NT_AS && *route != NT_AS_F16)
        AS_REFUSE("%s: route %s: only the A-stationary kernels are served (NT_AS, NT_AS_F16: 16-bit operands, K 256 / 512, bf16 also 128 / 1024, N %% 32 == 0, N <= 1024, no forced tile kernel; as_flags bits 6 / 7 send K = 512, N = 256 to NT_CS)",
                  me, nt_route_text(*route));
    gemm_nt_as_plan(c.dtM, c.dtC, c.M, c.N, c.K, ea, plan);
    // outputs and side operands: every access of the epilogue is 16 bytes wide (vt: single elements)
    const void* tc[7] = {c.C, c.pre_out, c.aux, c.resid, c.q, c.k, x.pro_out};
    const char* tcn[7] = {"C", "pre_out", "aux", "resid", "q", "k", "pro_out"};
    for (int k = 0; k < 7; ++k)
        if ((uintptr_t)tc[k] % 16 != 0) AS_REFUSE("%s: misaligned %s (16-byte aligned)", me, tcn[k]);
    if ((uintptr_t)c.vt % esC != 0) AS_REFUSE("%s: misaligned vt (%d-byte aligned)", me, esC);
    if ((uintptr_t)c.addtab % 16 != 0) AS_REFUSE("%s: misaligned addtab (16-byte aligned)", me);
    const void* f4[8] = {c.bias, c.rowscale, x.ln_gamma, x.ln_beta, x.ln_mean, x.ln_rstd, x.pa_P, x.pa_Q};
    const char* f4n[8] = {"bias", "rowscale", "ln_gamma", "ln_beta", "ln_mean", "ln_rstd", "pa_P", "pa_Q"};
    for (int k = 0; k < 8; ++k)
        if ((uintptr_t)f4[k] % 4 != 0) AS_REFUSE("%s: misaligned %s (4-byte aligned)", me, f4n[k]);
    return 0;
#undef AS_REFUSE
}

extern "C" int ishara_op_gemm_as(const ishara_gemm_nt_call* call, const ishara_gemm_as_ext* ext, ishara_stream st) {
    const char* me = "ishara_op_gemm_as";
    if (!call || !ext) { ishara_set_error("%s: null %s", me, call ? "ext" : "call"); return -1; }
    NtRoute route;
    AsPlan plan;
    if (as_call_refused(me, *call, *ext, &route, &plan)) return -1;
    const NtCall& c = *call;
    const EpiArgs ea = as_call_epi(c, *ext);
    const OpArgs oa = nt_call_op(c);
    return launch_gemm_nt(c.dtA, c.dtM, c.dtC, c.op, c.A, c.Bt, c.C, c.M, c.N, c.K, c.ldb, oa, ea, (hipStream_t)st);
}

extern "C" int ishara_debug_gemm_as_plan(const ishara_gemm_nt_call* call, const ishara_gemm_as_ext* ext, ishara_gemm_as_plan* out) {
    const char* me = "ishara_debug_gemm_as_plan";
    if (!call || !ext || !out) { ishara_set_error("%s: null argument", me); return -1; }
    *out = ishara_gemm_as_plan{};
    out->route = "NT_REFUSED"; out->kernel = "";
    NtRoute r;
    AsPlan p;
    if (as_call_refused(me, *call, *ext, &r, &p)) return 0;      // the reason is in ishara_last_error
    const EpiArgs ea = as_call_epi(*call, *ext);
    out->route = nt_route_text(r);
    out->kernel = gemm_nt_kernel_name(call->dtA, call->dtM, call->dtC, call->op, call->A, call->M, call->N, call->K, call->ldb, ea);
    out->rows = p.rows; out->gx = p.gx; out->gy = p.gy; out->nsteps = p.nsteps; out->ring = p.ring; out->cs = p.cs; out->waves = p.waves;
    out->passes = p.passes; out->pass_rows[0] = p.pass_rows[0]; out->pass_rows[1] = p.pass_rows[1];
    out->chunked = p.chunked; out->hold = p.hold; out->inst_mask = p.inst; out->prologue = p.pro;
    return 0;
}
