"""The A-stationary GEMM family (gemm_as.hip: gemm_nt_as_kernel, gemm_nt_as_chunk_kernel; gemm_as_f16.hip: the same source with fp16 operands)
through the handle-free entry ishara_op_gemm_as against int64 / fp64 numpy: case table, inputs, references, bounds, fingerprint operands and the
device runner shared by test_gemm_as_plan.py (CPU), test_gemm_as_mutants.py (CPU) and test_gemm_as_gpu.py.  Storage rounding, the dropout masks,
worst_ratio, GUARD / SENTINEL and TOL are those of gemm_nt_parity.py.

Exact form.  Operands and epilogue inputs are small integers in their storage type (A, Wt in [-4, 4], bias / PE table / residual in [-8, 8], the
act' operand in [-2, 2]), the row scale is one of 1, 2, 4, the dropout rate is 0.5 (scale exactly 2), act is none or ReLU, dact is DACT_POS, the
per-sample affine has P in {-2, -1, 1, 2} and integer Q in [-2, 2].  Every partial sum and every epilogue intermediate is then an integer below
2^24 in magnitude and the transformed operand is an integer a 16-bit type holds (test_gemm_as_plan.py asserts both per case): fp32 gives the same
value in any summation order, and the fp64 reference rounded ONCE to dtC must be array_equal to C, pre_out, q, k, vt and pro_out.

Real-valued form.  The same cases with N(0, 1) operands rounded to storage under the bound of gemm_nt_parity.py,
  |err[m, n]| <= 2 K 2^-24 (|A'| |Wt|^T + every epilogue addend's magnitude)[m, n] + u(dtC) |ref[m, n]|,
A' the operand as the kernel multiplies it.  The affine keeps P a power of two, so A * P + Q is one fp32 rounding however the compiler contracts it
and the reference rounds fp32 -> operand type as the kernel does: pro_out stays array_equal.  Swish / dSwish cases use TOL of test_ops_gpu.py.

LayerNorm prologue (real-valued only: no exact form exists).  Two separate checks.  (1) ln_mean, ln_rstd and pro_out against fp64 LayerNorm under
ln_bounds: the kernel sums the row's K values in fp32 (8 K / 32 per lane, then two shuffles), subtracts, squares and sums again, takes
rsqrt(q / K + eps), and forms (x - mean) * rstd * gamma + beta in fp32 before ONE rounding to the operand type.  With u = 2^-24:
    e_mean = K u mean|x| ;  d_var = (2 e_mean sum|x - mean| + (K + 3) u sum (x - mean)^2) / (K (var + eps)) + u
    |ln_mean - mean| <= e_mean ;  |ln_rstd - rstd| <= rstd (d_var / 2 + u + RSQ_ALLOW)
    |pro_out - y|    <= |gamma| rstd e_mean + |y - beta| (3 u + d_var / 2 + u + RSQ_ALLOW) + u |y| + u(operand type) |y|
RSQ_ALLOW is the one term that is measured, not derived: the relative accuracy of the hardware reciprocal square root (v_rsq_f32).  Observed on
the MI355X over every LayerNorm case of this table: the worst |ln_rstd - rstd| / rstd was RSQ_OBSERVED = 4.2e-7 (the whole error of ln_rstd, the
derived part included); the allowance is twice that, on top of the derived terms.  (2) C, pre_out, q, k, vt against the fp64 product of the DEVICE's own pro_out with the weights, under the GEMM bound above: the GEMM
part keeps its tight bound whatever the prologue's error.

Guards and poison.  Every output — C, pre_out, q, k, vt, pro_out, ln_mean, ln_rstd — sits between GUARD sentinel floats, and C / pre_out are
compared as whole [M, ldc] buffers in which the gap columns [N, ldc) and the columns [n_valid, N) must still hold the sentinel.  Bt has exactly N
rows; a case with ldb_pad has NaN in its columns [K, ldb); bias past n_valid is NaN — the contract in api_gemm_nt.hip: none of these is ever read.

Fingerprint operands (bf16 C, no bias; every value an integer <= 99).  a(m) = 1 + (m + m div 64) mod 3, A[m, k] = a(m) / K.
"step": Wt[n, k] = 1 + n div 32, so C[m, n] = a(m) (1 + n div 32) names the column step whose weights were multiplied;
"lane": Wt[n, k] = 1 + n mod 32, so C[m, n] = a(m) (1 + n mod 32) names the staged weight row.  decode(c, value, m, n) turns an element back into
the step (or weight row) under the row's own a(m), and into the a of the activations under the column's own weights."""
import ctypes as C
import functools
import zlib
from collections import namedtuple

import numpy as np

import gemm_nt_parity as G
from ishara_amd import _lib

store, round_bf16, cpu_masks, worst_ratio = G.store, G.round_bf16, G.cpu_masks, G.worst_ratio
GUARD, SENTINEL, TOL, U, UC, DT, ACT, DACT, SEED, EPI_SITE = G.GUARD, G.SENTINEL, G.TOL, G.U, G.UC, G.DT, G.ACT, G.DACT, G.SEED, G.EPI_SITE
RESID, M_DACT, M_ACT, DROP, ROWSCALE, PREOUT, QKV, ADDTAB, ALL = 1, 2, 4, 8, 16, 32, 64, 128, 255           # gemm_as.hip: AS_RESID .. AS_ALL
SMALL_M, MID_M_K512, CHUNK_ROWS, NS = 1536, 32768, 384, 32
LN_EPS = 1e-5
RSQ_OBSERVED = 4.2e-7        # worst |ln_rstd - rstd| / rstd seen on the MI355X over the LayerNorm cases of this table (4.175e-7: ln_chunk)
RSQ_ALLOW = 2.0 * RSQ_OBSERVED

# dt: the operand type (A, Bt, pro_out); pro: "none" / "ln" / "pa"; stats: ln_mean / ln_rstd wanted; like: the case whose inputs (and reference)
# this one shares — the paired-store rows differ in as_flags only; fp: "step" / "lane"; op: always "none" (cpu_masks reads it)
Case = namedtuple("Case", "name M N K dt dtC bias tab pre_out act drop rowscale dact resid qkv T pro pro_out stats ldc n_valid as_flags ldb_pad fp like "
                          "real_only op props")


def case(name, M, N, K, props, dt="bf16", dtC=None, bias=True, tab=0, pre_out=False, act="none", drop=False, rowscale=0, dact="none", resid=False,
         qkv=None, T=0, pro="none", pro_out=None, stats=None, ldc=0, n_valid=0, as_flags=51, ldb_pad=0, fp=None, like=None):
    if fp:
        bias = False
    if pro_out is None:
        pro_out = pro != "none"
    if stats is None:
        stats = pro == "ln"
    real_only = "swish" in (act, dact) or pro == "ln"
    return Case(name, M, N, K, dt, dtC or dt, bias, tab, pre_out, act, drop, rowscale, dact, resid, qkv, T, pro, pro_out, stats, ldc, n_valid, as_flags,
                ldb_pad, fp, like or name, real_only, "none", tuple(props.split()))


def with_mask(mask, **kw):
    """the case keywords that set exactly the features of an epilogue mask (ReLU / DACT_POS; T = 24 for the row scale)"""
    d = dict(resid=bool(mask & RESID), dact="pos" if mask & M_DACT else "none", act="relu" if mask & M_ACT else "none", drop=bool(mask & DROP),
             rowscale=1 if mask & ROWSCALE else 0, pre_out=bool(mask & PREOUT), tab=72 if mask & ADDTAB else 0)
    if mask & ROWSCALE:
        d["T"] = 24
    if mask & QKV:
        d.update(qkv=(2, 16, 1), T=8)
    d.update(kw)
    return d


BF16_MASKS = [0, RESID, RESID | ROWSCALE, ROWSCALE, RESID | DROP, M_ACT | PREOUT, M_ACT | PREOUT | DROP, M_ACT | DROP, M_ACT, M_DACT, M_DACT | DROP, QKV, ADDTAB]
F16_MASKS = [0, RESID, M_ACT | PREOUT, M_ACT, QKV, ADDTAB]
LN_MASKS = [0, M_ACT | PREOUT, M_ACT | PREOUT | DROP, QKV]
PA_MASKS = [RESID, RESID | ROWSCALE]
FLAGS = [0, 1, 3, 51]


def _cases():
    out = []
    add = out.append
    # ---- K and ring depth x column steps per workgroup, every row block full (counted waits): without a split on a store-only and on a loading mask
    for K in (256, 512):
        for n, (M, N) in {1: (128, 32), 2: (1664, 64), 3: (128, 96), 4: (1664, 128), 5: (128, 160)}.items():
            add(case(f"k{K}_n{n}", M, N, K, f"k{K}_n{n}_gy1_counted"))
            add(case(f"k{K}_n{n}_resid", M, N, K, f"k{K}_n{n}_gy1_loading", resid=True))
        # ... and reached through a column split (blockIdx.y redoes the prologue): counted with two stores per group, and loading
        for n, (M, N) in {1: (128, 64), 2: (64, 1024), 3: (128, 192), 4: (1664, 512), 5: (128, 320)}.items():
            kw = dict(pre_out=True, act="relu") if K == 256 else dict(dact="pos")
            add(case(f"k{K}_n{n}_split", M, N, K, f"k{K}_n{n}_split", **kw))
    for n, (M, N) in {1: (256, 32), 2: (1664, 64), 3: (256, 96), 5: (130, 160)}.items():
        add(case(f"k1024_n{n}", M, N, 1024, f"k1024_n{n}", resid=n % 2 == 0))
    add(case("k128_dact", 200, 96, 128, "k128_dact", dact="pos"))
    add(case("k128_dact_drop", 200, 96, 128, "k128_dact_drop", dact="pos", drop=True))
    add(case("k128_all", 200, 96, 128, "k128_all", resid=True))
    # ---- row forms at their M thresholds; the 192-row form's last workgroup
    add(case("k256_m1536", 1536, 64, 256, "k256_rows64_at_1536"))
    add(case("k256_m1537", 1537, 64, 256, "k256_rows128_at_1537", resid=True))
    add(case("k512_m32768", 32768, 32, 512, "k512_rows64_at_32768"))
    add(case("k512_m32769", 32769, 32, 512, "k512_rows192_at_32769 k512_last129", resid=True))
    add(case("k512_last100", 192 * 171 + 100, 64, 512, "k512_last100", pre_out=True, act="relu"))
    add(case("k512_last128", 192 * 171 + 128, 32, 512, "k512_last128", dact="pos"))
    add(case("k512_last192", 192 * 172, 64, 512, "k512_last192"))
    # ---- partial row blocks (full is false: every wait is vmcnt(0), the clamped rows store nothing) on store-only and loading masks
    for r in (1, 15, 16, 17, 63):
        for tag, kw in (("plain", {}), ("preout", dict(pre_out=True, act="relu")), ("resid", dict(resid=True)), ("dact", dict(dact="pos"))):
            add(case(f"k256_mod{r}_{tag}", 64 + r, 96, 256, f"rows64_mod{r}_{tag}", **kw))
    for i, r in enumerate((1, 15, 16, 17, 63)):
        kw = [{}, dict(resid=True), dict(pre_out=True, act="relu"), dict(dact="pos"), dict(resid=True)][i]
        add(case(f"k256_rows128_mod{r}", 1664 + r, 64, 256, f"rows128_mod{r}", **kw))
        add(case(f"k512_mod{r}", 64 + r, 96, 512, f"k512_rows64_mod{r}", **[dict(dact="pos"), {}, dict(resid=True), {}, dict(pre_out=True, act="relu")][i]))
    # ---- paired stores: as_flags 0, 1, 3, 51 on an odd and an even step count, with and without pre_out, at both ring depths, full row blocks
    for K in (256, 512):
        for par, (M, N) in (("odd", (128, 96)), ("even", (1664, 128))):
            for po in (False, True):
                base = f"hold_k{K}_{par}{'_preout' if po else ''}"
                for f in FLAGS:
                    add(case(f"{base}_f{f}", M, N, K, f"hold_k{K}_{par}_{'preout' if po else 'plain'}_f{f}", pre_out=po, act="relu" if po else "none", as_flags=f, like=f"{base}_f0"))
    add(case("hold_off_n_valid", 128, 64, 256, "hold_off_n_valid", n_valid=56, as_flags=1))
    # ---- the chunked kernel: 1, 2, 3 stages at K = 256 (a 100-row last workgroup), 2 and 3 at K = 512 with 100, 256, 257 and 384 rows in the last one
    add(case("chunk_k256_s1", 49252, 128, 256, "chunk_k256_stages1"))
    add(case("chunk_k256_s2", 49252, 256, 256, "chunk_k256_stages2", resid=True))
    add(case("chunk_k256_s3", 49153, 384, 256, "chunk_k256_stages3", pre_out=True, act="relu", drop=True))
    add(case("chunk_k512_last100", 49252, 128, 512, "chunk_k512_stages2 chunk_k512_last100", resid=True))
    add(case("chunk_k512_last256", 49408, 128, 512, "chunk_k512_last256", dact="pos", drop=True))
    add(case("chunk_k512_last257", 49409, 192, 512, "chunk_k512_stages3 chunk_k512_last257"))
    add(case("chunk_k512_last384", 49536, 128, 512, "chunk_k512_last384", pre_out=True, act="relu"))
    add(case("chunk_not_split", 49152, 256, 256, "chunk_fallback_split"))
    add(case("chunk_not_n_valid", 49252, 128, 256, "chunk_fallback_n_valid", n_valid=120))
    add(case("chunk_not_stages", 49252, 160, 256, "chunk_fallback_stages", resid=True))
    add(case("chunk_not_flag", 49252, 128, 256, "chunk_fallback_flag", as_flags=3))
    # ---- every compiled instantiation of run_as at a two-step shape (QKV: three steps), a partial last row block
    for K in (256, 512):
        for m in BF16_MASKS:
            add(case(f"mask{m}_k{K}", 1672, 96 if m & QKV else 64, K, f"bf16_mask{m}_k{K}", **with_mask(m)))
        add(case(f"all_resid_act_k{K}", 1669, 64, K, f"bf16_all_k{K}", **with_mask(RESID | M_ACT)))
    add(case("all_addtab_drop", 1669, 64, 256, "bf16_all_addtab_drop", **with_mask(ADDTAB | DROP)))
    add(case("all_dact_resid", 1669, 64, 256, "bf16_all_dact_resid", **with_mask(M_DACT | RESID)))
    add(case("all_qkv_rowscale", 1672, 96, 512, "bf16_all_qkv", **with_mask(QKV | ROWSCALE, T=8)))
    add(case("f32c_plain", 1669, 64, 256, "f32c_mask0", dtC="f32"))
    add(case("f32c_all", 1669, 64, 512, "f32c_all", dtC="f32", **with_mask(RESID | M_ACT | PREOUT)))
    add(case("f32c_all_dact_drop", 200, 96, 256, "f32c_all_dact", dtC="f32", **with_mask(M_DACT | DROP)))
    for K in (256, 512):
        for m in F16_MASKS:
            add(case(f"f16_mask{m}_k{K}", 1672, 96 if m & QKV else 64, K, f"f16_mask{m}_k{K}", dt="f16", **with_mask(m)))
    add(case("f16_all", 1669, 64, 256, "f16_all", dt="f16", **with_mask(RESID | M_ACT)))
    add(case("f16_f32c_plain", 200, 96, 512, "f16_f32c_mask0", dt="f16", dtC="f32"))
    add(case("f16_f32c_all", 1669, 64, 256, "f16_f32c_all", dt="f16", dtC="f32", resid=True))
    add(case("f16_hold_odd", 128, 96, 256, "f16_hold", dt="f16", pre_out=True, act="relu"))
    # ---- epilogue features at their own edges
    add(case("qkv_hm1_dh8", 160, 96, 256, "qkv_hm1_dh8", qkv=(4, 8, 1), T=40))
    add(case("qkv_hm0_dh32", 160, 96, 512, "qkv_hm0_dh32", qkv=(1, 32, 0), T=40))
    add(case("qkv_hm0_dh8", 1680, 192, 256, "qkv_hm0_dh8", qkv=(8, 8, 0), T=40))
    add(case("qkv_hm1_dh32", 160, 192, 256, "qkv_hm1_dh32", qkv=(2, 32, 1), T=40))
    add(case("addtab_period", 200, 96, 256, "addtab_period", tab=72))
    add(case("rowscale_value", 192, 96, 256, "rowscale_value", rowscale=1, T=24))
    add(case("rowscale_bias", 192, 96, 512, "rowscale_bias", rowscale=2, T=24, resid=True))
    add(case("n_valid60_ldc64", 200, 64, 256, "n_valid60_ldc64", dtC="f32", n_valid=60, ldc=64))
    add(case("n_valid60_ldc72", 200, 64, 512, "n_valid60_ldc72", dtC="f32", n_valid=60, ldc=72))
    add(case("n_valid60_f16", 130, 64, 256, "n_valid60_f16", dt="f16", dtC="f32", n_valid=60, ldc=60))
    add(case("ldc_gap_bf16", 1669, 64, 256, "ldc_gap_bf16", ldc=80, pre_out=True, act="relu"))
    add(case("ldb_pad", 200, 96, 256, "ldb_pad", ldb_pad=64, resid=True))
    add(case("swish_preout", 200, 96, 256, "swish", pre_out=True, act="swish"))
    add(case("dswish_k512", 1669, 64, 512, "dswish", dact="swish"))
    add(case("f16_swish", 200, 96, 256, "f16_swish", dt="f16", act="swish"))
    # ---- per-sample affine prologue: T = the rows per workgroup of each row form (every workgroup another sample) and twice that; both masks;
    # with and without pro_out; under a column split (only blockIdx.y == 0 writes pro_out)
    add(case("pa_rows64", 64 * 5 + 10, 96, 256, "pa_rows64_T1", T=64, pro="pa", **with_mask(RESID)))
    add(case("pa_rows64_T2", 64 * 5, 96, 256, "pa_rows64_T2 pa_no_pro_out", pro="pa", pro_out=False, **with_mask(RESID | ROWSCALE, T=128)))
    add(case("pa_rows128", 128 * 13 + 20, 64, 256, "pa_rows128_T1", pro="pa", **with_mask(RESID | ROWSCALE, T=128)))
    add(case("pa_rows128_T2", 128 * 13, 64, 256, "pa_rows128_T2", T=256, pro="pa", **with_mask(RESID)))
    add(case("pa_k512_rows64", 64 * 4 + 33, 96, 512, "pa_k512_rows64_T1", T=64, pro="pa", **with_mask(RESID)))
    add(case("pa_k512_rows192", 192 * 171 + 129, 32, 512, "pa_k512_rows192_T1", pro="pa", **with_mask(RESID | ROWSCALE, T=192)))
    add(case("pa_k512_rows192_T2", 192 * 172, 32, 512, "pa_k512_rows192_T2", T=384, pro="pa", pro_out=False, **with_mask(RESID)))
    add(case("pa_k1024", 128 * 3 + 5, 96, 1024, "pa_k1024", T=128, pro="pa", **with_mask(RESID)))
    add(case("pa_split", 128, 64, 256, "pa_split", T=64, pro="pa", **with_mask(RESID)))
    add(case("pa_split_k512", 1664, 512, 512, "pa_split_k512", pro="pa", **with_mask(RESID | ROWSCALE, T=64)))
    add(case("pa_f16", 64 * 3 + 7, 96, 256, "pa_f16", dt="f16", T=64, pro="pa", **with_mask(RESID)))
    add(case("pa_chunk_k256", 49536, 128, 256, "pa_chunk_k256", T=384, pro="pa", **with_mask(RESID)))
    add(case("pa_chunk_k512", 49152 + 257, 128, 512, "pa_chunk_k512", pro="pa", **with_mask(RESID | ROWSCALE, T=384)))
    # ---- LayerNorm prologue: the four compiled masks at K = 256 and 512 (N = 64 at few rows: a column split), one without a split, one chunked
    for K in (256, 512):
        for m in LN_MASKS:
            add(case(f"ln_mask{m}_k{K}", 200, 96 if m & QKV else 64, K, f"ln_mask{m}_k{K}", pro="ln", **with_mask(m, T=40 if m & QKV else 0)))
    add(case("ln_nosplit", 1669, 64, 256, "ln_nosplit", pro="ln", pre_out=True, act="relu"))
    add(case("ln_k1024", 200, 96, 1024, "ln_k1024", pro="ln"))
    add(case("ln_f16", 200, 96, 512, "ln_f16", dt="f16", pro="ln", pre_out=True, act="relu"))
    add(case("ln_chunk", 49252, 128, 256, "ln_chunk", pro="ln"))
    add(case("ln_no_outputs", 200, 96, 256, "ln_no_outputs", pro="ln", pro_out=False, stats=False))
    # ---- fingerprints: a pair per ring depth and a pair on the chunked kernel
    for fp in ("step", "lane"):
        add(case(f"fp_{fp}_k256", 1671, 160, 256, f"fp_{fp}_ring3", fp=fp))
        add(case(f"fp_{fp}_k512", 1671, 160, 512, f"fp_{fp}_ring2", fp=fp))
        add(case(f"fp_{fp}_chunk", 49252, 256, 256, f"fp_{fp}_chunk", fp=fp))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
EXACT_CASES = [c for c in CASES if not c.real_only]
REAL_CASES = [c for c in CASES if not c.fp]
LN_CASES = [c for c in CASES if c.pro == "ln"]


# ------------------------------------------------------------------ the plan the rows claim: a mirror of gemm_nt_as_plan that test_gemm_as_plan.py
# holds, field by field, to ishara_debug_gemm_as_plan
Plan = namedtuple("Plan", "route kernel rows gx gy nsteps ring cs waves passes pass_rows chunked hold inst pro")


def mask_of(c):
    return ((RESID if c.resid else 0) | (M_DACT if c.dact != "none" else 0) | (M_ACT if c.act != "none" else 0) | (DROP if c.drop else 0) |
            (ROWSCALE if c.rowscale else 0) | (PREOUT if c.pre_out else 0) | (QKV if c.qkv else 0) | (ADDTAB if c.tab else 0))


def inst_mask(c):
    m = mask_of(c)
    if c.pro != "none":
        return m if m in (LN_MASKS if c.pro == "ln" else PA_MASKS) and c.dtC == c.dt and c.K >= 256 else -1
    if c.dtC == "f32":
        return 0 if m == 0 else ALL
    if c.K == 128:
        return m if m in (M_DACT, M_DACT | DROP) else ALL
    return m if m in (F16_MASKS if c.dt == "f16" else BF16_MASKS) else ALL


@functools.lru_cache(maxsize=None)
def plan(name):
    c = BY_NAME[name]
    M, N, K, kt = c.M, c.N, c.K, c.K // 32
    br = (64 if M <= SMALL_M else 128) if kt <= 8 else ((64 if M <= MID_M_K512 else 192) if kt <= 16 else 128)
    gx, slots = -(-M // br), (768 if kt <= 8 else (512 if kt <= 16 else 256))
    gy, max_gy, min_cols = 1, (16 if M <= SMALL_M else 4), (32 if M <= SMALL_M else 128)
    while gy < max_gy and gx * gy * 2 <= slots and (N // NS) % (gy * 2) == 0 and N // (gy * 2) >= min_cols:
        gy *= 2
    inst, pro = inst_mask(c), {"none": 0, "ln": 1, "pa": 2}[c.pro]
    cs = 4 if K == 256 else 2
    chunked = (c.dt == "bf16" and c.dtC == "bf16" and inst not in (-1, ALL) and bool(c.as_flags & 16 if K == 256 else (K == 512 and c.as_flags & 32)) and
               M >= 128 * CHUNK_ROWS and (N // NS) % cs == 0 and N >= 128 and not c.n_valid and (c.pro != "pa" or c.T % CHUNK_ROWS == 0) and gy == 1)
    hold = c.dtC != "f32" and c.dtC == c.dt and inst not in (-1, ALL) and not inst & QKV and bool(c.as_flags & 1) and not c.n_valid
    ct = "bf16" if c.dtC == "bf16" else "f32"
    if c.dt == "f16":
        kernel = "gemm_nt_kernel<f16>"
    elif chunked:
        kernel = f"gemm_nt_as_chunk_kernel<bf16,{kt},{inst},{pro}>"
    else:
        kernel = f"gemm_nt_as_kernel<{ct},{kt},{inst},0,{pro}>" if pro else f"gemm_nt_as_kernel<{ct},{kt},{inst},0>"
    route = "NT_AS_F16" if c.dt == "f16" else "NT_AS"
    if chunked:
        return Plan(route, kernel, CHUNK_ROWS, -(-M // CHUNK_ROWS), 1, N // NS, 2, cs, 12 if K == 256 else 8, 1 if K == 256 else 2,
                    (384, 0) if K == 256 else (256, 128), 1, int(hold), inst, pro)
    return Plan(route, kernel, br, gx, gy, N // NS // gy, 3 if kt <= 8 else 2, 1, 4 if kt <= 16 else 8, 2 if br == 192 else 1,
                (128, 64) if br == 192 else (br, 0), 0, int(hold), inst, pro)


def locate(c, m, n):
    """where the kernel computes element (m, n): workgroup (x, y), pass, wave, 16-row tile of the wave, column step of the workgroup, ring slot"""
    p = plan(c.name)
    x, r = divmod(m, p.rows)
    ps = 0 if r < p.pass_rows[0] else 1
    r -= p.pass_rows[0] * ps
    rt = p.pass_rows[ps] // (16 * p.waves)               # row tiles per wave
    y, nn = divmod(n, p.nsteps * NS)
    s = nn // NS
    return dict(x=x, y=y, ps=ps, wave=r // (16 * rt), tile=r % (16 * rt) // 16, step=s, slot=(s // p.cs) % p.ring, sub=s % p.cs)


def last_rows(c):
    """rows of the last workgroup"""
    p = plan(c.name)
    return c.M - (p.gx - 1) * p.rows


# property -> predicate over the case and its plan; every property needs a case, every case keeps its own (test_gemm_as_plan.py)
def _p(c):
    return plan(c.name)


def _full(c):
    return c.M % _p(c).rows == 0


def _counted(c):
    return mask_of(c) & (RESID | M_DACT | ADDTAB | QKV) == 0


def _ring(K):
    return 3 if K <= 256 else 2


def _props():
    P = {}
    for K in (256, 512):
        for n in (1, 2, 3, 4, 5):
            P[f"k{K}_n{n}_gy1_counted"] = lambda c, K=K, n=n: c.K == K and _p(c).ring == _ring(K) and _p(c).nsteps == n and _p(c).gy == 1 and _full(c) and _counted(c) and not _p(c).chunked
            P[f"k{K}_n{n}_gy1_loading"] = lambda c, K=K, n=n: c.K == K and _p(c).nsteps == n and _p(c).gy == 1 and _full(c) and not _counted(c) and not _p(c).chunked
            P[f"k{K}_n{n}_split"] = lambda c, K=K, n=n: c.K == K and _p(c).nsteps == n and _p(c).gy > 1 and _full(c) and _counted(c) == (K == 256)
    for n in (1, 2, 3, 5):
        P[f"k1024_n{n}"] = lambda c, n=n: c.K == 1024 and _p(c).ring == 2 and _p(c).waves == 8 and _p(c).rows == 128 and _p(c).nsteps == n and _p(c).gy == 1
    P["k128_dact"] = lambda c: c.K == 128 and _p(c).ring == 3 and _p(c).inst == M_DACT
    P["k128_dact_drop"] = lambda c: c.K == 128 and _p(c).inst == (M_DACT | DROP)
    P["k128_all"] = lambda c: c.K == 128 and _p(c).inst == ALL and mask_of(c) != ALL
    P["k256_rows64_at_1536"] = lambda c: c.K == 256 and c.M == SMALL_M and _p(c).rows == 64
    P["k256_rows128_at_1537"] = lambda c: c.K == 256 and c.M == SMALL_M + 1 and _p(c).rows == 128
    P["k512_rows64_at_32768"] = lambda c: c.K == 512 and c.M == MID_M_K512 and _p(c).rows == 64 and _p(c).passes == 1
    P["k512_rows192_at_32769"] = lambda c: c.K == 512 and c.M == MID_M_K512 + 1 and _p(c).rows == 192 and _p(c).pass_rows == (128, 64)
    for r in (100, 128, 129, 192):
        P[f"k512_last{r}"] = lambda c, r=r: c.K == 512 and _p(c).rows == 192 and not _p(c).chunked and last_rows(c) == r
    for r in (1, 15, 16, 17, 63):
        for tag, mk in (("plain", 0), ("preout", M_ACT | PREOUT), ("resid", RESID), ("dact", M_DACT)):
            P[f"rows64_mod{r}_{tag}"] = lambda c, r=r, mk=mk: c.K == 256 and _p(c).rows == 64 and c.M % 64 == r and c.M > 64 and mask_of(c) == mk and _p(c).nsteps > 2
        P[f"rows128_mod{r}"] = lambda c, r=r: c.K == 256 and _p(c).rows == 128 and c.M % 128 == r and _p(c).gx > 1
        P[f"k512_rows64_mod{r}"] = lambda c, r=r: c.K == 512 and _p(c).rows == 64 and c.M % 64 == r and c.M > 64 and _p(c).nsteps > 2
    for K in (256, 512):
        for par in ("odd", "even"):
            for po in ("plain", "preout"):
                for f in FLAGS:
                    P[f"hold_k{K}_{par}_{po}_f{f}"] = (lambda c, K=K, par=par, po=po, f=f: c.K == K and c.as_flags == f and _p(c).hold == (f & 1) and _full(c) and _p(c).gy == 1 and
                                                       _p(c).nsteps > 2 and _p(c).nsteps % 2 == (par == "odd") and c.pre_out == (po == "preout") and _counted(c) and
                                                       not _p(c).chunked and c.like == c.name[:c.name.rindex("_f")] + "_f0")
    P["hold_off_n_valid"] = lambda c: c.as_flags & 1 and c.n_valid and c.dtC == "bf16" and _p(c).inst == 0 and not _p(c).hold
    for s in (1, 2, 3):
        P[f"chunk_k256_stages{s}"] = lambda c, s=s: c.K == 256 and _p(c).chunked and _p(c).cs == 4 and _p(c).waves == 12 and _p(c).nsteps == 4 * s and _p(c).gy == 1 and c.M >= 49153 and _p(c).ring == 2
    for s in (2, 3):
        P[f"chunk_k512_stages{s}"] = lambda c, s=s: c.K == 512 and _p(c).chunked and _p(c).cs == 2 and _p(c).waves == 8 and _p(c).nsteps == 2 * s and _p(c).pass_rows == (256, 128)
    for r in (100, 256, 257, 384):
        P[f"chunk_k512_last{r}"] = lambda c, r=r: c.K == 512 and _p(c).chunked and last_rows(c) == r
    P["chunk_fallback_split"] = lambda c: c.M == 49152 and c.K == 256 and _p(c).gy > 1 and not _p(c).chunked and c.as_flags & 16 and c.N % 128 == 0
    P["chunk_fallback_n_valid"] = lambda c: c.M > 49152 and c.K == 256 and c.n_valid and not _p(c).chunked and c.as_flags & 16 and c.N % 128 == 0 and _p(c).gy == 1
    P["chunk_fallback_stages"] = lambda c: c.M > 49152 and c.K == 256 and (c.N // 32) % 4 != 0 and c.N >= 128 and not _p(c).chunked and c.as_flags & 16 and _p(c).gy == 1
    P["chunk_fallback_flag"] = lambda c: c.M > 49152 and c.K == 256 and c.N % 128 == 0 and not c.as_flags & 16 and not _p(c).chunked
    for K in (256, 512):
        for m in BF16_MASKS:
            P[f"bf16_mask{m}_k{K}"] = lambda c, K=K, m=m: c.K == K and c.dt == "bf16" and c.dtC == "bf16" and c.pro == "none" and _p(c).inst == m == mask_of(c) and _p(c).nsteps == (3 if m & QKV else 2) and c.M % _p(c).rows
        for m in F16_MASKS:
            P[f"f16_mask{m}_k{K}"] = lambda c, K=K, m=m: c.K == K and c.dt == "f16" and c.dtC == "f16" and _p(c).inst == m == mask_of(c) and _p(c).nsteps == (3 if m & QKV else 2) and _p(c).route == "NT_AS_F16"
        P[f"bf16_all_k{K}"] = lambda c, K=K: c.K == K and c.dtC == "bf16" and _p(c).inst == ALL and _p(c).nsteps == 2
    P["bf16_all_addtab_drop"] = lambda c: c.dtC == "bf16" and _p(c).inst == ALL and mask_of(c) == ADDTAB | DROP
    P["bf16_all_dact_resid"] = lambda c: c.dtC == "bf16" and _p(c).inst == ALL and mask_of(c) == M_DACT | RESID
    P["bf16_all_qkv"] = lambda c: c.dtC == "bf16" and _p(c).inst == ALL and mask_of(c) & QKV
    P["f32c_mask0"] = lambda c: c.dt == "bf16" and c.dtC == "f32" and _p(c).inst == 0 and _p(c).nsteps == 2
    P["f32c_all"] = lambda c: c.dt == "bf16" and c.dtC == "f32" and _p(c).inst == ALL and _p(c).nsteps == 2 and c.pre_out
    P["f32c_all_dact"] = lambda c: c.dt == "bf16" and c.dtC == "f32" and _p(c).inst == ALL and c.dact == "pos" and c.drop
    P["f16_all"] = lambda c: c.dt == "f16" and c.dtC == "f16" and _p(c).inst == ALL
    P["f16_f32c_mask0"] = lambda c: c.dt == "f16" and c.dtC == "f32" and _p(c).inst == 0
    P["f16_f32c_all"] = lambda c: c.dt == "f16" and c.dtC == "f32" and _p(c).inst == ALL
    P["f16_hold"] = lambda c: c.dt == "f16" and _p(c).hold and _p(c).nsteps % 2 == 1 and c.pre_out and _full(c)
    for hm in (0, 1):
        for dh in (8, 32):
            P[f"qkv_hm{hm}_dh{dh}"] = lambda c, hm=hm, dh=dh: c.qkv and c.qkv[1:] == (dh, hm) and c.T % 8 == 0 and c.T % _p(c).rows != 0 and _p(c).inst == QKV
    P["addtab_period"] = lambda c: 0 < c.tab < c.M and _p(c).rows % c.tab != 0 and c.tab % _p(c).rows != 0 and _p(c).inst == ADDTAB
    P["rowscale_value"] = lambda c: c.rowscale == 1 and c.bias and c.T % _p(c).rows != 0
    P["rowscale_bias"] = lambda c: c.rowscale == 2 and c.bias and c.T % _p(c).rows != 0
    P["n_valid60_ldc64"] = lambda c: (c.n_valid, c.N, c.ldc) == (60, 64, 64) and c.bias
    P["n_valid60_ldc72"] = lambda c: (c.n_valid, c.N, c.ldc) == (60, 64, 72) and c.bias
    P["n_valid60_f16"] = lambda c: (c.n_valid, c.N, c.ldc, c.dt) == (60, 64, 60, "f16")
    P["ldc_gap_bf16"] = lambda c: c.ldc > c.N and c.dtC == "bf16" and c.pre_out and not c.n_valid and _p(c).hold
    P["ldb_pad"] = lambda c: c.ldb_pad > 0
    P["swish"] = lambda c: c.act == "swish" and c.pre_out and c.dt == "bf16"
    P["dswish"] = lambda c: c.dact == "swish"
    P["f16_swish"] = lambda c: c.act == "swish" and c.dt == "f16"
    pa = lambda c, rows, k: c.pro == "pa" and c.K == k and _p(c).rows == rows and not _p(c).chunked and _p(c).gx > 2          # noqa: E731
    P["pa_rows64_T1"] = lambda c: pa(c, 64, 256) and c.T == 64 and c.pro_out and mask_of(c) == RESID and c.M % 64
    P["pa_rows64_T2"] = lambda c: pa(c, 64, 256) and c.T == 128 and mask_of(c) == RESID | ROWSCALE
    P["pa_no_pro_out"] = lambda c: c.pro == "pa" and not c.pro_out
    P["pa_rows128_T1"] = lambda c: pa(c, 128, 256) and c.T == 128 and mask_of(c) == RESID | ROWSCALE and c.M % 128
    P["pa_rows128_T2"] = lambda c: pa(c, 128, 256) and c.T == 256
    P["pa_k512_rows64_T1"] = lambda c: pa(c, 64, 512) and c.T == 64
    P["pa_k512_rows192_T1"] = lambda c: pa(c, 192, 512) and c.T == 192 and last_rows(c) == 129
    P["pa_k512_rows192_T2"] = lambda c: pa(c, 192, 512) and c.T == 384
    P["pa_k1024"] = lambda c: pa(c, 128, 1024) and c.T == 128
    P["pa_split"] = lambda c: c.pro == "pa" and c.K == 256 and _p(c).gy > 1 and c.pro_out and c.T == _p(c).rows and _p(c).gx > 1
    P["pa_split_k512"] = lambda c: c.pro == "pa" and c.K == 512 and _p(c).gy > 1 and c.pro_out and c.T == _p(c).rows and _p(c).nsteps > 2
    P["pa_f16"] = lambda c: c.pro == "pa" and c.dt == "f16" and c.T == _p(c).rows
    P["pa_chunk_k256"] = lambda c: c.pro == "pa" and c.K == 256 and _p(c).chunked and c.T == 384
    P["pa_chunk_k512"] = lambda c: c.pro == "pa" and c.K == 512 and _p(c).chunked and c.T == 384 and last_rows(c) > 256
    for K in (256, 512):
        for m in LN_MASKS:
            P[f"ln_mask{m}_k{K}"] = lambda c, K=K, m=m: c.pro == "ln" and c.K == K and _p(c).inst == m == mask_of(c) and c.pro_out and c.stats and c.M % _p(c).rows and (_p(c).gy > 1 or m & QKV)
    P["ln_nosplit"] = lambda c: c.pro == "ln" and _p(c).gy == 1 and _p(c).rows == 128 and not _p(c).chunked
    P["ln_k1024"] = lambda c: c.pro == "ln" and c.K == 1024
    P["ln_f16"] = lambda c: c.pro == "ln" and c.dt == "f16"
    P["ln_chunk"] = lambda c: c.pro == "ln" and _p(c).chunked
    P["ln_no_outputs"] = lambda c: c.pro == "ln" and not c.pro_out and not c.stats
    for fp in ("step", "lane"):
        P[f"fp_{fp}_ring3"] = lambda c, fp=fp: c.fp == fp and c.K == 256 and _p(c).ring == 3 and _p(c).nsteps == 5 and _p(c).gy == 1 and not _p(c).chunked and c.dtC == "bf16"
        P[f"fp_{fp}_ring2"] = lambda c, fp=fp: c.fp == fp and c.K == 512 and _p(c).ring == 2 and _p(c).nsteps == 5 and _p(c).gy == 1 and not _p(c).chunked and c.dtC == "bf16"
        P[f"fp_{fp}_chunk"] = lambda c, fp=fp: c.fp == fp and _p(c).chunked and _p(c).nsteps == 8 and c.dtC == "bf16"
    return P


PROPS = _props()


# ------------------------------------------------------------------ inputs
def fp_row_factor(m):
    m = np.asarray(m)
    return 1 + (m + m // 64) % 3


def qkv_dims(c):
    H, dh, hm = c.qkv
    return c.M // c.T, H, dh, hm


def nsamples(c):
    return -(-c.M // c.T)


def inputs(name, real):
    """the operands of a case as fp64 arrays holding values of the storage types (the case's `like` names whose: cases that differ in as_flags
    only share them)"""
    return _inputs(BY_NAME[name].like, bool(real))


@functools.lru_cache(maxsize=3)
def _inputs(name, real):
    c = BY_NAME[name]
    g = np.random.default_rng(zlib.crc32(c.name.encode()) * 2 + int(real))
    op = {}

    def draw(shape, lo, hi, dt):
        return store(g.standard_normal(shape), dt) if real else g.integers(lo, hi + 1, shape).astype(np.float64)

    if c.fp:
        op["A"] = np.repeat((fp_row_factor(np.arange(c.M)) / c.K)[:, None], c.K, 1)
        w = 1 + np.arange(c.N) // NS if c.fp == "step" else 1 + np.arange(c.N) % NS
        op["W"] = np.repeat(w.astype(np.float64)[:, None], c.K, 1)
        return op
    op["W"] = draw((c.N, c.K), -4, 4, c.dt)
    if c.pro == "ln":            # rows with their own mean in [-3, 3], |x| up to 8
        op["A"] = store(np.clip(2.0 * g.standard_normal((c.M, c.K)) + g.uniform(-3, 3, (c.M, 1)), -8, 8), c.dt)
        op["gamma"] = store(1.0 + 0.25 * g.standard_normal(c.K), "f32")
        op["beta"] = store(0.5 * g.standard_normal(c.K), "f32")
    else:
        op["A"] = draw((c.M, c.K), -4, 4, c.dt)
    if c.pro == "pa":            # P a power of two in both forms (see the head of the file); neighbouring samples differ
        nb = nsamples(c)
        op["P"] = g.choice([-2.0, -1.0, 1.0, 2.0], (nb, c.K)) * (g.choice([0.5, 1.0, 2.0], (nb, c.K)) if real else 1.0)
        op["Q"] = draw((nb, c.K), -2, 2, "f32")
    if c.bias:
        op["bias"] = draw(c.N, -8, 8, "f32")
    if c.tab:
        op["addtab"] = draw((c.tab, c.N), -8, 8, "f32")
    if c.rowscale:
        op["rowscale"] = g.choice([1.0, 2.0, 4.0], nsamples(c))
        op["rowscale"][:3] = g.permutation([1.0, 2.0, 4.0])[: len(op["rowscale"][:3])]
    if c.dact != "none":
        op["aux"] = draw((c.M, c.N), -2, 2, c.dtC)
    if c.resid:
        op["resid"] = draw((c.M, c.N), -8, 8, c.dtC)
    return op


# ------------------------------------------------------------------ reference, magnitudes, bounds, mutants
MUTANTS = ["stale_weights", "held_at_odd_columns", "last_odd_step_dropped", "second_pass_dropped", "clamp_off_by_one", "split_overlap", "no_pair_permutation",
           "pa_neighbour_sample", "bias_past_n_valid", "rowscale_modes_swapped", "qkv_layouts_swapped"]


def mutant_applies(c, mut):
    p = plan(c.name)
    return {
        "stale_weights": p.nsteps // p.cs > p.ring,
        "held_at_odd_columns": bool(p.hold) and p.nsteps >= 2,
        "last_odd_step_dropped": bool(p.hold) and p.nsteps % 2 == 1,
        "second_pass_dropped": p.passes == 2 and last_rows(c) > p.pass_rows[0],
        "clamp_off_by_one": c.M > 1,
        "split_overlap": p.gy > 1,
        "no_pair_permutation": c.dtC != "f32",
        "pa_neighbour_sample": c.pro == "pa",
        "bias_past_n_valid": bool(c.n_valid) and c.bias,
        "rowscale_modes_swapped": bool(c.rowscale) and c.bias,
        "qkv_layouts_swapped": bool(c.qkv),
    }[mut]


def layernorm64(c, op):
    """fp64 LayerNorm of the rows: mean, rstd, y (unrounded)"""
    x = op["A"]
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    return mean, rstd, (x - mean[:, None]) * rstd[:, None] * op["gamma"][None, :] + op["beta"][None, :]


def staged(c, op, mut=None):
    """A as the kernel multiplies it: transformed in fp32, rounded ONCE to the operand type"""
    A = op["A"]
    if c.pro == "pa":
        b = np.arange(c.M) // c.T
        if mut == "pa_neighbour_sample":
            b = (b + 1) % nsamples(c)
        A = store((A * op["P"][b] + op["Q"][b]).astype(np.float32).astype(np.float64), c.dt)
    elif c.pro == "ln":
        A = store(layernorm64(c, op)[2], c.dt)
    return A


def _scatter(c, v, hm):
    B, H, dh, _ = qkv_dims(c)
    x = v.reshape(B, c.T, H, 3, dh) if hm else v.reshape(B, c.T, 3, H, dh).transpose(0, 1, 3, 2, 4)
    return [x[:, :, :, i, :].transpose(0, 2, 1, 3) for i in range(3)]       # [B, H, T, dh]


def compute(c, op, masks, absolute=False, mut=None, a_staged=None):
    """the logical outputs of the call in fp64 before the rounding to dtC: C [M, N] (or q, k, vt), pre_out, and with a prologue pro_out [M, K].
    absolute: every factor and addend replaced by its magnitude and every gate open — the sums that bound every intermediate and scale the error
    bound.  mut: one ordinary mistake; an element the mistaken kernel never stores holds SENTINEL.  a_staged: the operand to multiply instead of
    the reference's own (the LayerNorm cases: the device's pro_out)"""
    f = np.abs if absolute else (lambda x: x)
    p = plan(c.name)
    M, N = c.M, c.N
    A = f(staged(c, op, mut) if a_staged is None else a_staged)
    W = f(op["W"])
    acc = A @ W.T
    sent = SENTINEL[c.dtC]
    wg_rows = slice((p.gx - 1) * p.rows, M)                    # the last workgroup's rows
    width = p.nsteps * NS                                      # columns of one split
    if mut == "stale_weights":          # the last workgroup of the last split multiplies, at its last step, the weights the slot held a lap earlier
        s = p.nsteps - 1
        s_old = s - p.ring * p.cs
        n0 = (p.gy - 1) * width
        acc[wg_rows, n0 + s * NS:n0 + (s + 1) * NS] = A[wg_rows] @ W[n0 + s_old * NS:n0 + (s_old + 1) * NS].T
    if mut == "clamp_off_by_one":
        acc[M - 1] = acc[M - 2]
    if mut == "split_overlap":          # the last split stages the weight rows from one step below its own
        n0 = (p.gy - 1) * width
        acc[:, n0:n0 + width] = A @ W[n0 - NS:n0 - NS + width].T
    if mut == "no_pair_permutation":    # columns 4..7 and 8..11 of every 16 exchanged in the accumulators
        idx = np.arange(N)
        j = idx % 16
        acc = acc[:, np.where((j >= 4) & (j < 8), idx + 4, np.where((j >= 8) & (j < 12), idx - 4, idx))]
    rows = np.arange(M)
    rsb = c.rowscale == 2
    if mut == "rowscale_modes_swapped" and c.rowscale:
        rsb = not rsb
    rs = f(op["rowscale"])[rows // c.T][:, None] if c.rowscale else None
    v = acc
    if c.bias:
        b = np.broadcast_to(np.nan_to_num(f(op["bias"]))[None, :], (M, N))
        v = v + (b * rs if c.rowscale and rsb else b)
    if c.tab:
        v = v + f(op["addtab"])[rows % c.tab]
    out = {}
    if c.pre_out:
        out["pre_out"] = v
    if c.act == "relu" and not absolute:
        v = np.maximum(v, 0.0)
    elif c.act == "swish":
        v = v if absolute else v / (1.0 + np.exp(-v))
    if c.drop:
        v = v * masks["epi"]
    if c.rowscale and not rsb:
        v = v * rs
    if c.dact == "pos" and not absolute:
        v = np.where(op["aux"] > 0, v, 0.0)
    elif c.dact == "swish":
        a = op["aux"]
        s = 1.0 / (1.0 + np.exp(-a))
        v = v * (np.abs(s * (1.0 + a * (1.0 - s))) if absolute else s * (1.0 + a * (1.0 - s)))
    if c.resid:
        v = v + f(op["resid"])
    if c.pro != "none" and c.pro_out:
        out["pro_out"] = A
    if c.qkv:
        B, H, dh, hm = qkv_dims(c)
        q, k, vv = _scatter(c, v, 1 - hm if mut == "qkv_layouts_swapped" else hm)
        out["q"], out["k"], out["vt"] = np.ascontiguousarray(q), np.ascontiguousarray(k), np.ascontiguousarray(vv.transpose(0, 1, 3, 2))
        return out
    out["C"] = v
    both = ["C"] + (["pre_out"] if c.pre_out else [])
    if mut == "held_at_odd_columns":    # the last workgroup stores its first held group at the odd step's columns: the even step's are never written
        for n in both:
            out[n] = out[n].copy()
            out[n][wg_rows, NS:2 * NS] = out[n][wg_rows, 0:NS]
            out[n][wg_rows, 0:NS] = sent
    if mut == "last_odd_step_dropped":
        for n in both:
            out[n] = out[n].copy()
            out[n][:, (p.nsteps - 1) * NS:p.nsteps * NS] = sent
    if mut == "second_pass_dropped":
        for n in both:
            out[n] = out[n].copy()
            out[n][(p.gx - 1) * p.rows + p.pass_rows[0]:] = sent
    return out


def layout(c, outs, fill, rounded, mut=None):
    """the buffers the call leaves: C and pre_out as [M, ldc] with `fill` (the sentinel; 0 for a bound) in the gap columns [N, ldc) and in the
    columns [n_valid, N); every 16/32-bit output rounded once to its type when `rounded`"""
    res = {}
    ldc, nv = (c.ldc or c.N), (c.n_valid or c.N)
    for n, v in outs.items():
        dt = c.dt if n == "pro_out" else ("f32" if n in ("ln_mean", "ln_rstd") else c.dtC)
        w = store(v, dt) if rounded else np.asarray(v, np.float64)          # (the sentinel of a mutant's unwritten element is a value of the type)
        if n in ("C", "pre_out") and (c.ldc or c.n_valid):
            full = np.full((c.M, ldc), float(fill))
            full[:, :nv] = w[:, :nv]
            if mut == "bias_past_n_valid":          # the bias is not cleared past n_valid and the column guard is left out: the NaN there is stored
                full[:, nv:min(c.N, ldc)] = np.nan
            w = full
        res[n] = w
    return res


def reference(c, op, masks, mut=None, rounded=True, a_staged=None):
    """what the call must leave in every output buffer: fp64, rounded once to the output's type (exact form: the comparison is array_equal)"""
    return layout(c, compute(c, op, masks, False, mut, a_staged), SENTINEL[c.dtC], rounded, mut)


def magnitudes(c, op, masks, a_staged=None):
    return compute(c, op, masks, True, None, a_staged)


def bounds(c, op, masks, a_staged=None):
    """elementwise 2 K 2^-24 * magnitude + u(dtC) * |ref|; pro_out of the affine prologue: 0 (array_equal); the untouched columns: 0"""
    ref, mag = compute(c, op, masks, False, None, a_staged), magnitudes(c, op, masks, a_staged)
    b = {n: (np.zeros_like(ref[n]) if n == "pro_out" else 2.0 * c.K * U * mag[n] + UC[c.dtC] * np.abs(ref[n])) for n in ref}
    return layout(c, b, 0.0, False)


def ln_reference(c, op):
    """fp64 LayerNorm outputs and their derived bounds (the head of the file): name -> (reference, bound) for ln_mean, ln_rstd, pro_out"""
    x, K = op["A"], c.K
    mean, rstd, y = layernorm64(c, op)
    d = x - mean[:, None]
    e_mean = K * U * np.abs(x).mean(1)
    d_var = (2.0 * e_mean * np.abs(d).sum(1) + (K + 3) * U * (d * d).sum(1)) / (K * ((d * d).mean(1) + LN_EPS)) + U
    rel = d_var / 2.0 + U + RSQ_ALLOW
    t = np.abs(y - op["beta"][None, :])
    b_y = np.abs(op["gamma"])[None, :] * (rstd * e_mean)[:, None] + t * (3.0 * U + rel)[:, None] + (U + UC[c.dt]) * np.abs(y)
    return {"ln_mean": (mean, e_mean + U * np.abs(mean)), "ln_rstd": (rstd, rstd * rel), "pro_out": (y, b_y)}


def expected(name, real):
    """(reference, bounds or None) of a case on its own inputs with the oracle's masks; kept for the runs that follow each other (the paired-store
    rows of one group share it through `like`).  The real-valued reference is not rounded to dtC: the bound carries that rounding"""
    return _expected(BY_NAME[name].like, bool(real))


@functools.lru_cache(maxsize=3)
def _expected(name, real):
    c, op = BY_NAME[name], inputs(name, real)
    m = cpu_masks(c)
    return reference(c, op, m, rounded=not real), (bounds(c, op, m) if real else None)


def decode(c, value, m, n):
    """a fingerprint element read back: {"weights": the column step ("step") or staged weight row ("lane") whose weights give `value` with the row's
    own activations, "a": the a(m') of the activations that give it with the column's own weights}; None where no integer fits"""
    w_own = (1 + n // NS) if c.fp == "step" else (1 + n % NS)
    a_own = int(fp_row_factor(m))
    ok = np.isfinite(value) and value > 0 and value == int(value)
    wq = value / a_own - 1 if ok else None
    aq = value / w_own if ok else None
    return {"weights": int(wq) if ok and wq == int(wq) and 0 <= wq < max(c.N // NS, NS) else None, "a": int(aq) if ok and aq == int(aq) and 1 <= aq <= 3 else None}


def element_of(c, name, idx):
    """output index -> the GEMM's (m, n)"""
    if name in ("C", "pre_out"):
        return idx
    B, H, dh, hm = qkv_dims(c)
    b, h, t, i = idx if name != "vt" else (idx[0], idx[1], idx[3], idx[2])
    part = ("q", "k", "vt").index(name)
    return b * c.T + t, (h * 3 * dh + part * dh + i) if hm else (part * H * dh + h * dh + i)


def describe_wrong(c, name, got, want, limit=6):
    """the first wrong elements of output `name` of an exact case: (m, n), the workgroup (x, y), the pass, wave and row tile, the column step and
    ring slot, got, want and, for a fingerprint case, which step's (or staged row's) weights and which a(m) of activations were multiplied"""
    got, want = np.asarray(got, np.float64), np.asarray(want)
    bad = np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))
    box = " x ".join(f"{int(lo)}..{int(hi)}" for lo, hi in zip(bad.min(0), bad.max(0)))
    p = plan(c.name)
    lines = [f"{c.name} {name}: {len(bad)} wrong elements of {want.size}, all inside index box {box}; plan rows {p.rows} grid ({p.gx}, {p.gy}) nsteps {p.nsteps} "
             f"ring {p.ring} cs {p.cs} chunked {p.chunked} hold {p.hold} inst {p.inst} pro {p.pro}"]
    for idx in bad[:limit]:
        idx = tuple(int(i) for i in idx)
        g, w = float(got[idx]), float(want[idx])
        if name in ("pro_out", "ln_mean", "ln_rstd"):
            lines.append(f"  {name}{list(idx)} workgroup x {idx[0] // p.rows} got {g!r} want {w!r}")
            continue
        m, n = element_of(c, name, idx)
        if n >= c.N:
            lines.append(f"  ({m}, {n}) in the gap columns [N, ldc) got {g!r} want the sentinel {w!r}")
            continue
        L = locate(c, m, n)
        s = (f"  ({m}, {n}) workgroup ({L['x']}, {L['y']}) pass {L['ps']} wave {L['wave']} row tile {L['tile']} step {L['step']} slot {L['slot']}"
             + (f" sub {L['sub']}" if p.cs > 1 else "") + f" got {g!r} want {w!r}")
        if c.fp:
            d, key = decode(c, g, m, n), ("step" if c.fp == "step" else "weight row")
            own = n // NS if c.fp == "step" else n % NS
            s += f" weights of {key} {d['weights']} (want {own}), activations a {d['a']} (want {int(fp_row_factor(m))})"
        lines.append(s)
    return "\n".join(lines)


# ------------------------------------------------------------------ the library: plan and device run
def _fake(i):
    return 4096 * (i + 1)


def buffers(c):
    """the pointer fields the case sets: (call fields, ext fields)"""
    names = ["A", "Bt"] + (["C"] if not c.qkv else ["q", "k", "vt"])
    names += (["bias"] if c.bias else []) + (["addtab"] if c.tab else []) + (["pre_out"] if c.pre_out else []) + (["rowscale"] if c.rowscale else [])
    names += (["aux"] if c.dact != "none" else []) + (["resid"] if c.resid else [])
    ext = {"ln": ["ln_gamma", "ln_beta"], "pa": ["pa_P", "pa_Q"], "none": []}[c.pro] + (["pro_out"] if c.pro_out and c.pro != "none" else [])
    ext += ["ln_mean", "ln_rstd"] if c.stats and c.pro == "ln" else []
    return names, ext


def ldb(c):
    return c.K + c.ldb_pad


def make_call(c, ptrs=None):
    """(ishara_gemm_nt_call, ishara_gemm_as_ext) of a case; ptrs: name -> address (default: made-up aligned addresses for everything the case has)"""
    names, ext = buffers(c)
    if ptrs is None:
        ptrs = {n: _fake(i) for i, n in enumerate(names + ext)}
    k, x = _lib.GemmNtCall(), _lib.GemmAsExt()
    for n in names:
        setattr(k, n, ptrs[n])
    for n in ext:
        setattr(x, n, ptrs[n])
    k.dtA = k.dtM = DT[c.dt]
    k.dtC, k.op = DT[c.dtC], 0
    k.M, k.N, k.K, k.bt_rows, k.ldb = c.M, c.N, c.K, c.N, ldb(c)
    k.tab_period, k.act = (c.tab or 1), ACT[c.act]
    k.drop_seed, k.drop_site, k.drop_rate = SEED, EPI_SITE, (0.5 if c.drop else 0.0)
    k.T, k.rowscale_bias, k.dact = (c.T or 1), int(c.rowscale == 2), DACT[c.dact]
    k.mode, k.H, k.dh, k.head_major = (1, *c.qkv) if c.qkv else (0, 1, 1, 1)
    x.ln_eps, x.ldc, x.n_valid, x.as_flags = LN_EPS, c.ldc, c.n_valid, c.as_flags
    return k, x


def lib_plan(lib, c):
    """the Plan of the case from ishara_debug_gemm_as_plan (host only); a refused call: route "NT_REFUSED", the message in ishara_last_error"""
    k, x = make_call(c)
    p = _lib.GemmAsPlan()
    rc = lib.ishara_debug_gemm_as_plan(C.byref(k), C.byref(x), C.byref(p))
    assert rc == 0, lib.ishara_last_error()
    return Plan(p.route.decode(), p.kernel.decode(), p.rows, p.gx, p.gy, p.nsteps, p.ring, p.cs, p.waves, p.passes, tuple(p.pass_rows), p.chunked, p.hold,
                p.inst_mask, p.prologue)


def out_shapes(c):
    """name -> (shape, storage type) of every buffer the call writes"""
    s = {}
    if c.qkv:
        B, H, dh, _ = qkv_dims(c)
        s["q"] = s["k"] = ((B, H, c.T, dh), c.dtC)
        s["vt"] = ((B, H, dh, c.T), c.dtC)
    else:
        s["C"] = ((c.M, c.ldc or c.N), c.dtC)
    if c.pre_out:
        s["pre_out"] = ((c.M, c.ldc or c.N), c.dtC)
    if c.pro != "none" and c.pro_out:
        s["pro_out"] = ((c.M, c.K), c.dt)
    if c.pro == "ln" and c.stats:
        s["ln_mean"] = s["ln_rstd"] = ((c.M,), "f32")
    return s


class Device:
    """the inputs of one case on the device (uploaded once), and fresh guarded outputs per launch"""
    def __init__(self, lib, c, op):
        import torch
        self.lib, self.c, self.torch = lib, c, torch
        self.tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

        def up(x, dt):
            return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.tdt[dt]).to("cuda")

        Bt = np.full((c.N, ldb(c)), np.nan)               # exactly N rows; the columns [K, ldb) are never read
        Bt[:, :c.K] = op["W"]
        self.t = {"A": up(op["A"], c.dt), "Bt": up(Bt, c.dt)}
        for n, dt in (("addtab", "f32"), ("rowscale", "f32"), ("aux", c.dtC), ("resid", c.dtC)):
            if n in op:
                self.t[n] = up(op[n], dt)
        if c.bias:
            b = op["bias"].copy()
            if c.n_valid:
                b[c.n_valid:] = np.nan
            self.t["bias"] = up(b, "f32")
        for n, src in (("ln_gamma", "gamma"), ("ln_beta", "beta"), ("pa_P", "P"), ("pa_Q", "Q")):
            if src in op:
                self.t[n] = up(op[src], "f32")

    def masks(self):
        torch, c, m = self.torch, self.c, {}
        if c.drop:
            t = torch.empty(c.M, c.N, dtype=torch.float32, device="cuda")
            _lib.check(self.lib.ishara_dropout_mask(SEED, EPI_SITE, c.M, c.N, C.c_float(0.5), C.c_void_p(t.data_ptr()), _lib.stream()), "ishara_dropout_mask")
            torch.cuda.synchronize()
            m["epi"] = t.cpu().numpy().astype(np.float64)
        return m

    def launch(self):
        """one launch into fresh outputs between sentinels; returns name -> fp32 array (C / pre_out: the whole [M, ldc] buffer), plus "guards_ok" """
        torch, c = self.torch, self.c
        outs = {}
        for n, (shape, dt) in out_shapes(c).items():
            es = 4 if dt == "f32" else 2
            g, k = GUARD * 4 // es, int(np.prod(shape))
            outs[n] = (torch.full((k + 2 * g,), SENTINEL[dt], dtype=self.tdt[dt], device="cuda"), k, g, es, dt)
        ptrs = {n: v.data_ptr() for n, v in self.t.items()}
        ptrs.update({n: v.data_ptr() + g * es for n, (v, _, g, es, _) in outs.items()})
        call, ext = make_call(c, ptrs)
        rc = self.lib.ishara_op_gemm_as(C.byref(call), C.byref(ext), _lib.stream())
        _lib.check(rc, "ishara_op_gemm_as")
        torch.cuda.synchronize()
        r = {"guards_ok": True}
        for n, (v, k, g, _, dt) in outs.items():
            sent = SENTINEL[dt]
            r["guards_ok"] = r["guards_ok"] and bool((v[:g] == sent).all().item()) and bool((v[g + k:] == sent).all().item())
            r[n] = v[g:g + k].float().cpu().numpy().reshape(out_shapes(c)[n][0])
        return r
