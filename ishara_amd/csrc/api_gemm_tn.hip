// Handle-free entry points of the weight-gradient GEMM family (gemm_tn.hip, gemm_big.hip): ishara_op_gemm_tn runs a list of calls through
// launch_gemm_tn as the models' gemm_wgrad does, at once or with the deferred slab sums; ishara_debug_gemm_tn_plan reports the route and split
// plan of one call from gemm_tn_plan, the function the launcher launches from.
#include <string>
#include "kernels.h"

typedef ishara_gemm_tn_call TnCall;

static bool tn_call_has_psa(const TnCall& c) { return c.psa_T != 0 || c.P || c.Q || c.W || c.G || c.Rpart; }
static TnPsa tn_call_psa(const TnCall& c) {
    TnPsa p; p.P = c.P; p.Q = c.Q; p.W = c.W; p.ldw = c.ldw; p.G = c.G; p.Rpart = c.Rpart; p.T = c.psa_T;
    return p;
}
static TnPlan tn_call_plan(const TnCall& c) {
    const TnPsa psa = tn_call_psa(c);
    return gemm_tn_plan(c.dtA, c.dtB, c.dtM, OP_NONE, OP_NONE, c.A, c.B, c.dbias != nullptr, c.M, c.Ka, c.Nb, c.ka_valid, c.nb_valid,
                        c.bias_rowscale, c.bias_T, tn_call_has_psa(c) ? &psa : nullptr);
}
// the dtypes of a call: each known, none fp16
static bool tn_call_dt_ok(const char* me, int i, const TnCall& c) {
    const int dts[3] = {c.dtA, c.dtB, c.dtM};
    const char* names[3] = {"dtA", "dtB", "dtM"};
    for (int k = 0; k < 3; ++k) {
        if (dts[k] != DT_F32 && dts[k] != DT_BF16 && dts[k] != DT_F16) {
            ishara_set_error("%s: call %d: unknown dtype %s=%d (ISHARA_F32 = 0, ISHARA_BF16 = 1, ISHARA_F16 = 2)", me, i, names[k], dts[k]); return false;
        }
        if (dts[k] == DT_F16) { ishara_set_error("%s: call %d: %s: ISHARA_F16 is inference-only (no fp16 weight-gradient kernels)", me, i, names[k]); return false; }
    }
    return true;
}
// everything about call i that a launch would fault or fail on, before any HIP call: the entry's own checks (buffers), then the launcher's (its message)
static int tn_call_refused(const char* me, int i, const TnCall& c, TnPlan* plan_out) {
    if (!tn_call_dt_ok(me, i, c)) return -1;
    if (!c.A || !c.B || !c.out) { ishara_set_error("%s: call %d: null A / B / out", me, i); return -1; }
    if (((uintptr_t)c.out | (uintptr_t)c.dbias | (uintptr_t)c.bias_rowscale | (uintptr_t)c.P | (uintptr_t)c.Q | (uintptr_t)c.G | (uintptr_t)c.Rpart) % 4 != 0 ||
        (uintptr_t)c.W % 2 != 0) {
        ishara_set_error("%s: call %d: misaligned buffer (out, dbias, bias_rowscale, P, Q, G, Rpart: 4-byte aligned; W: 2-byte aligned)", me, i); return -1;
    }
    const TnPlan plan = tn_call_plan(c);           // refuses a bad shape, a misaligned A / B and every call gemm_tn_route refuses
    if (plan.route == TN_REFUSED) {                // the launcher's message, behind the entry's name and the call's index
        const char* le = ishara_last_error();
        const std::string why = le ? le : "";
        ishara_set_error("%s: call %d: %s", me, i, why.c_str());
        return -1;
    }
    if (plan.route == TN_TR_PSA && c.ldw < c.Nb) { ishara_set_error("%s: call %d: ldw=%d < Nb=%d (W is [Ka][ldw])", me, i, c.ldw, c.Nb); return -1; }
    if (plan.splits <= 0 || plan.rps <= 0) { ishara_set_error("%s: call %d: internal error: route without a split plan", me, i); return -1; }
    const size_t stride = (size_t)c.Ka * c.Nb + c.Nb;
    if ((size_t)plan.splits * stride > gemm_tn_slab_floats(c.M, c.Ka, c.Nb, c.dtM)) {
        ishara_set_error("%s: call %d: the plan's %d splits do not fit the slab (gemm_tn_slab_floats)", me, i, plan.splits); return -1;
    }
    if (plan_out) *plan_out = plan;
    return 0;
}

extern "C" int64_t ishara_op_gemm_tn_scratch_bytes(const ishara_gemm_tn_call* calls, int32_t n) {
    if (!calls || n < 1) return -1;
    size_t floats = 0;
    for (int i = 0; i < n; ++i) {
        const TnCall& c = calls[i];
        if (c.M < 1 || c.Ka < 1 || c.Nb < 1 || (c.dtM != DT_F32 && c.dtM != DT_BF16)) return -1;
        const size_t f = gemm_tn_slab_floats(c.M, c.Ka, c.Nb, c.dtM);
        if (f > floats) floats = f;
    }
    return (int64_t)(floats * sizeof(float));
}

extern "C" int ishara_op_gemm_tn(const ishara_gemm_tn_call* calls, int32_t n, void* slab, void* defer_slab0, void* defer_slab1, ishara_stream st) {
    const char* me = "ishara_op_gemm_tn";
    if (!calls || n < 1) { ishara_set_error("%s: null or empty call list (n=%d)", me, n); return -1; }
    if (!slab || (uintptr_t)slab % 16 != 0) { ishara_set_error("%s: null or misaligned slab (16-byte aligned, ishara_op_gemm_tn_scratch_bytes)", me); return -1; }
    if ((defer_slab0 != nullptr) != (defer_slab1 != nullptr)) { ishara_set_error("%s: deferred mode needs both defer_slab0 and defer_slab1", me); return -1; }
    if (((uintptr_t)defer_slab0 | (uintptr_t)defer_slab1) % 16 != 0) { ishara_set_error("%s: misaligned defer slab (16-byte aligned)", me); return -1; }
    if (defer_slab0 && (defer_slab0 == defer_slab1 || defer_slab0 == slab || defer_slab1 == slab)) { ishara_set_error("%s: slab, defer_slab0 and defer_slab1 must be three buffers", me); return -1; }
    for (int i = 0; i < n; ++i)
        if (tn_call_refused(me, i, calls[i], nullptr)) return -1;
    hipStream_t s = (hipStream_t)st;
    TnDefer defer;
    defer.slab[0] = (float*)defer_slab0; defer.slab[1] = (float*)defer_slab1;
    TnDefer* dp = defer_slab0 ? &defer : nullptr;
    OpArgs no;
    int rc = 0;
    for (int i = 0; i < n && rc == 0; ++i) {
        const TnCall& c = calls[i];
        const TnPsa psa = tn_call_psa(c);
        rc = launch_gemm_tn(c.dtA, c.dtB, c.dtM, OP_NONE, OP_NONE, c.A, c.B, c.out, c.dbias, (float*)slab, c.M, c.Ka, c.Nb, no, no, s,
                            c.ka_valid, c.nb_valid, c.bias_rowscale, c.bias_T, dp, tn_call_has_psa(c) ? &psa : nullptr);
    }
    const int frc = launch_gemm_tn_flush(dp, s);      // also after a failed call: what earlier calls left pending is summed
    return rc != 0 ? rc : frc;
}

extern "C" int ishara_debug_gemm_tn_plan(const ishara_gemm_tn_call* call, const char** route, const char** kernel, int32_t* splits, int32_t* rows_per_split) {
    const char* me = "ishara_debug_gemm_tn_plan";
    if (!call || !route || !kernel || !splits || !rows_per_split) { ishara_set_error("%s: null argument", me); return -1; }
    *route = "TN_REFUSED"; *kernel = ""; *splits = 0; *rows_per_split = 0;
    if (!tn_call_dt_ok(me, 0, *call)) return 0;
    const TnPlan p = tn_call_plan(*call);
    switch (p.route) {
        case TN_REFUSED: return 0;
        case TN_BIG: *route = "TN_BIG"; break;
        case TN_TR: *route = "TN_TR"; break;
        case TN_TR_BRS: *route = "TN_TR_BRS"; break;
        case TN_TR_PSA: *route = "TN_TR_PSA"; break;
        case TN_REG: *route = "TN_REG"; break;
    }
    const TnPsa psa = tn_call_psa(*call);
    *kernel = gemm_tn_kernel_name(call->dtA, call->dtB, call->dtM, OP_NONE, OP_NONE, call->M, call->Ka, call->Nb, call->ka_valid, call->nb_valid,
                                  call->bias_rowscale, call->bias_T, tn_call_has_psa(*call) ? &psa : nullptr);
    *splits = p.splits; *rows_per_split = p.rps;
    return 0;
}
