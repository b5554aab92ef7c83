"""The weight-gradient GEMM family (launch_gemm_tn: gemm_tn.hip, gemm_big.hip) against int64 / fp64 numpy: case tables, inputs, references,
bounds and the device runner shared by test_gemm_tn_plan.py (CPU), test_gemm_tn_mutants.py (CPU) and test_gemm_tn_gpu.py.

Exact form.  A, B, W are integers in [-2, 2] in their storage type, P, Q come from {-2, -1, -0.5, 0, 0.5, 1, 2}, the bias row scale from
{0, 1, 1.25} and out / dbias are pre-filled with integers.  Every product and every partial sum is then a multiple of 1/4 whose magnitude times
4 stays below 2^24 (test_gemm_tn_plan.py asserts it for every case, from the sums of absolute values), so the fp32 result is the same in any
summation order — in the MFMAs, across M-splits, in the slab sums, in the per-sample fold — and array_equal against the reference is legitimate.
The reference's matrix products run in fp64, which is exact for these integers (< 2^53).

Real-valued form.  The same cases with N(0, 1) operands rounded to the storage type (out / dbias pre-filled with zeros), held to the worst case
of fp32 summation in any order: |err[k, n]| <= c * M * 2^-24 * (|A|^T |B|)[k, n], c = 2 for plain sums (dW, dbias, G), c = 4 for the per-sample
fold and Rpart, whose magnitudes carry |P|, |Q|, |W| inside the product.  The mixed-type register-transposing kernels round their f32 operand
to bf16 while staging it (dtM = bf16): the reference rounds it the same way, so the bound measures the summation, not that rounding.  Their
bias gradient sums the f32 values as loaded, before that rounding, and so does the reference's."""
import ctypes as C
import functools
import zlib
from collections import namedtuple

import numpy as np

from ishara_amd import _lib

DT = {"f32": _lib.F32, "bf16": _lib.BF16}
U = 2.0 ** -24
GUARD = 64                    # floats behind every output that must come back untouched
SENTINEL = 77777.0
FORCE_TN_REG = 2              # ishara_debug_force_regstage: the register-transposing kernel
PQ_SET = np.array([-2, -1, -0.5, 0, 0.5, 1, 2])
RS_SET = np.array([0, 1, 1.25])

# brs_T / psa_T: 0 = no bias row scale / no per-sample-affine block; psa_rs: the PSA call also has a bias row scale (T = psa_T); nt_big 0: under
# ishara_debug_set_nt_big(0); refused: the launcher refuses the call (plan test and refusal tests only); props: what the case is in the table for
Case = namedtuple("Case", "name M Ka Nb dtA dtB ka_valid nb_valid bias brs_T psa_T psa_rs nt_big refused props")
Plan = namedtuple("Plan", "route kernel splits rps")


def case(name, M, Ka, Nb, props, dtA="bf16", dtB="bf16", ka_valid=0, nb_valid=0, bias=True, brs_T=0, psa_T=0, psa_rs=False, nt_big=1, refused=False):
    return Case(name, M, Ka, Nb, dtA, dtB, ka_valid, nb_valid, bias, brs_T, psa_T, psa_rs, nt_big, refused, tuple(props.split()))


CASES = [
    # ---- TN_TR: the split plan's edges (one 128 x 128 tile unless the row is about tiles)
    case("tr_m256", 256, 128, 128, "tr_1x8"),
    case("tr_m320", 320, 128, 128, "tr_1x10"),
    case("tr_m576", 576, 128, 128, "tr_2x9"),
    case("tr_m704", 704, 256, 128, "tr_2x11"),
    case("tr_m832", 832, 128, 256, "tr_3_short_last"),
    case("tr_m2048", 2048, 128, 128, "tr_x8_full_last"),
    case("tr_m2112", 2112, 256, 256, "tr_x8_last3"),
    case("tr_m4352", 4352, 128, 128, "tr_x8_last1"),
    case("tr_m1856", 1856, 128, 256, "tr_7_splits"),
    case("tr_m5184", 5184, 128, 128, "tr_search_x8"),
    case("tr_m4160", 4160, 128, 128, "tr_search_runs_out"),
    case("tr_m7936", 7936, 128, 128, "tr_one_stage_x8", bias=False),
    case("tr_n384", 832, 128, 384, "tr_3_tiles_row"),
    case("tr_24tiles", 4096, 512, 768, "tr_24_tiles_no_defer"),
    # ---- TN_TR_BRS: the weighted bias sum, samples of 1, 3 and 5 stages against splits that cut them
    case("brs_t32", 832, 128, 128, "brs_T32", brs_T=32),
    case("brs_t96", 960, 128, 256, "brs_T96", brs_T=96),
    case("brs_t160", 1280, 256, 128, "brs_T160", brs_T=160),
    case("brs_t48", 960, 128, 128, "brs_T_not_x32_refused", brs_T=48, refused=True),
    # ---- TN_TR_PSA: samples per split 1, 2, 3, 5, 7; several splits; with and without a bias row scale
    case("psa_b2", 2 * 128, 128, 128, "psa_ns2 psa_with_rowscale", psa_T=128, psa_rs=True),
    case("psa_b3", 3 * 128, 256, 128, "psa_ns3 psa_with_rowscale", psa_T=128, psa_rs=True),
    case("psa_b5", 5 * 128, 128, 256, "psa_ns5 psa_without_rowscale", psa_T=128),
    case("psa_b7", 7 * 128, 128, 128, "psa_ns7 psa_without_rowscale", psa_T=128, bias=False),
    case("psa_t256_b4", 4 * 256, 128, 128, "psa_ns1 psa_without_rowscale", psa_T=256),
    case("psa_b16", 16 * 128, 256, 256, "psa_multi_split psa_with_rowscale", psa_T=128, psa_rs=True),
    case("psa_b11", 11 * 128, 128, 128, "psa_refused_B11", psa_T=128, refused=True),
    case("psa_t96", 8 * 96, 128, 128, "psa_refused_T", psa_T=96, refused=True),
    # ---- zero-padded operands: the stem (276 real input columns of 384) and the classifier (60 real classes of 128)
    case("ka_valid_stem", 2112, 384, 128, "ka_valid_276_of_384", ka_valid=276, bias=False),
    case("nb_valid_cls", 704, 256, 128, "nb_valid_60_of_128", nb_valid=60),
    # ---- TN_REG: the four type combinations at M 1, 63, 65, 130, 2T - 1 = 299 and ragged widths (60 as f32 B, 276 as f32 A)
    case("reg_m1", 1, 8, 136, "reg_bf16_bf16 reg_M1 reg_dim8 reg_dim136"),
    case("reg_m130", 130, 136, 8, "reg_bf16_bf16 reg_M130 reg_dim8 reg_dim136"),
    case("reg_m299_fa", 299, 276, 136, "reg_f32_bf16 reg_M299 reg_dim276_f32A", dtA="f32"),
    case("reg_m65_fb", 65, 136, 60, "reg_bf16_f32 reg_M65 reg_dim60_f32B", dtB="f32"),
    case("reg_m63_ff", 63, 276, 60, "reg_f32_f32 reg_M63 reg_dim276_f32A reg_dim60_f32B", dtA="f32", dtB="f32"),
    case("reg_m299_ff", 299, 8, 136, "reg_f32_f32 reg_M299", dtA="f32", dtB="f32"),
    case("reg_m130_fb", 130, 8, 60, "reg_bf16_f32 reg_M130", dtB="f32"),
    case("reg_m65_fa", 65, 276, 8, "reg_f32_bf16 reg_M65", dtA="f32"),
    # ---- TN_BIG: the 256 x 256 tile kernel, and the transposed-read kernel it replaces at the same shape
    case("big", 32768, 512, 512, "big"),
    case("big_brs", 32768, 512, 512, "big_brs_T128", brs_T=128),
    case("big_off", 32768, 512, 512, "big_off_falls_to_tr", nt_big=0),
    case("big_off_brs", 32768, 512, 512, "big_off_falls_to_tr_brs", brs_T=128, nt_big=0),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUN_CASES = [c for c in CASES if not c.refused]
# the forced register kernel where the route allows: a plain transposed-read call (no bias row scale, per-sample affine or padding)
FORCED = [c for c in RUN_CASES if c.name.startswith("tr_")]

# Deferred chains: every call of a chain shares one deferred-sum state.  What each position is for (test_gemm_tn_plan.py asserts it):
#   chain "riders": two deferring calls of different tile counts (the second carries the first's sums as riders), a call that sums at once
#   (splits > 64) while carrying the second's, a TN_REG call (ignores the state), a deferring call, a PSA call (sums that call's slabs inline and
#   defers its own), a padded deferring call that carries the PSA call's sums, and a last deferring call whose sums are left for the flush
#   chain "big": two deferring calls, a TN_BIG call (flushes first), a deferring call left for the flush
CHAINS = {
    "riders": ["tr_m576", "tr_n384", "tr_m4160", "reg_m130", "tr_m1856", "psa_b16", "nb_valid_cls", "brs_t160"],
    "big": ["tr_m704", "tr_m2112", "big_brs", "ka_valid_stem"],
}


def dtm(c):
    """the MFMA operand type: f32 only for two f32 operands, as the models' calls have it"""
    return "f32" if c.dtA == "f32" and c.dtB == "f32" else "bf16"


def tiles(c):
    return ((c.Ka + 127) // 128) * ((c.Nb + 127) // 128)


def rows_of_splits(c, p):
    """rows of every M-split of the plan"""
    return [min(c.M, (i + 1) * p.rps) - i * p.rps for i in range(p.splits)]


def _stages(c, p):
    return [r // 32 for r in rows_of_splits(c, p)]


def _cuts_samples(c, p, T):
    """an M-split that starts and ends inside a sample"""
    return any((i * p.rps) % T != 0 and min(c.M, (i + 1) * p.rps) % T != 0 for i in range(p.splits))


def _tr(c, p):
    return p.route == "TN_TR" and p.kernel == "gemm_tn_tr_kernel<0>"


def _psa(c, p, ns=None, B=None, T=128):
    return (p.route == "TN_TR_PSA" and p.kernel == "gemm_tn_tr_kernel<0,false,true>" and c.psa_T == T and (B is None or c.M == B * T)
            and (ns is None or p.rps == ns * T))


def _reg(c, p, a, b):
    return p.route == "TN_REG" and (c.dtA, c.dtB) == (a, b) and p.kernel == f"gemm_tn_kernel<{a},{b},{dtm(c)}>"


# property -> predicate over (case, its plan as ishara_debug_gemm_tn_plan reports it); every property needs a case, every case keeps its own
PROPS = {
    "tr_1x8": lambda c, p: _tr(c, p) and _stages(c, p) == [8],
    "tr_1x10": lambda c, p: _tr(c, p) and _stages(c, p) == [10],
    "tr_2x9": lambda c, p: _tr(c, p) and _stages(c, p) == [9, 9],
    "tr_2x11": lambda c, p: _tr(c, p) and _stages(c, p) == [11, 11],
    "tr_3_short_last": lambda c, p: _tr(c, p) and p.splits == 3 and _stages(c, p)[2] < _stages(c, p)[0],
    "tr_x8_full_last": lambda c, p: _tr(c, p) and p.splits % 8 == 0 and len(set(_stages(c, p))) == 1 and _stages(c, p)[0] >= 8,
    "tr_x8_last3": lambda c, p: _tr(c, p) and p.splits % 8 == 0 and _stages(c, p)[-1] == 3 and _stages(c, p)[0] > 4,
    "tr_x8_last1": lambda c, p: _tr(c, p) and p.splits % 8 == 0 and _stages(c, p)[-1] == 1 and _stages(c, p)[0] >= 8,
    "tr_7_splits": lambda c, p: _tr(c, p) and p.splits == 7,
    # the launcher's first plan has at most M / 256 splits (8 stages each): more of them can only come out of its search loop
    "tr_search_x8": lambda c, p: _tr(c, p) and p.splits > c.M // 256 and p.splits % 8 == 0 and _stages(c, p)[0] > 1,
    "tr_search_runs_out": lambda c, p: _tr(c, p) and p.splits > 64 and p.splits % 8 != 0 and set(_stages(c, p)) == {1},
    "tr_one_stage_x8": lambda c, p: _tr(c, p) and p.splits > 64 and p.splits % 8 == 0 and set(_stages(c, p)) == {1},
    "tr_3_tiles_row": lambda c, p: _tr(c, p) and (c.Ka, c.Nb) == (128, 384),
    "tr_24_tiles_no_defer": lambda c, p: _tr(c, p) and c.M == 4096 and tiles(c) == 24 and tiles(c) * p.splits > 256,
    "brs_T32": lambda c, p: p.route == "TN_TR_BRS" and c.brs_T == 32 and p.splits > 1,
    "brs_T96": lambda c, p: p.route == "TN_TR_BRS" and c.brs_T == 96 and _cuts_samples(c, p, 96),
    "brs_T160": lambda c, p: p.route == "TN_TR_BRS" and c.brs_T == 160 and _cuts_samples(c, p, 160),
    "brs_T_not_x32_refused": lambda c, p: p.route == "TN_REFUSED" and c.brs_T % 32 != 0,
    "psa_ns1": lambda c, p: _psa(c, p, ns=1, B=4, T=256),
    "psa_ns2": lambda c, p: _psa(c, p, ns=2, B=2),
    "psa_ns3": lambda c, p: _psa(c, p, ns=3, B=3),
    "psa_ns5": lambda c, p: _psa(c, p, ns=5, B=5),
    "psa_ns7": lambda c, p: _psa(c, p, ns=7, B=7),
    "psa_multi_split": lambda c, p: _psa(c, p, B=16) and p.splits > 1,
    "psa_with_rowscale": lambda c, p: _psa(c, p, T=c.psa_T) and c.psa_rs,
    "psa_without_rowscale": lambda c, p: _psa(c, p, T=c.psa_T) and not c.psa_rs,
    "psa_refused_B11": lambda c, p: p.route == "TN_REFUSED" and c.psa_T == 128 and c.M == 11 * 128,
    "psa_refused_T": lambda c, p: p.route == "TN_REFUSED" and c.psa_T % 128 != 0 and c.M % c.psa_T == 0,
    "ka_valid_276_of_384": lambda c, p: _tr(c, p) and (c.ka_valid, c.Ka) == (276, 384),
    "nb_valid_60_of_128": lambda c, p: _tr(c, p) and (c.nb_valid, c.Nb) == (60, 128) and c.bias,
    "reg_bf16_bf16": lambda c, p: _reg(c, p, "bf16", "bf16"),
    "reg_f32_bf16": lambda c, p: _reg(c, p, "f32", "bf16"),
    "reg_bf16_f32": lambda c, p: _reg(c, p, "bf16", "f32"),
    "reg_f32_f32": lambda c, p: _reg(c, p, "f32", "f32"),
    **{f"reg_M{m}": (lambda c, p, m=m: p.route == "TN_REG" and c.M == m) for m in (1, 63, 65, 130, 299)},
    "reg_dim8": lambda c, p: p.route == "TN_REG" and 8 in (c.Ka, c.Nb),
    "reg_dim136": lambda c, p: p.route == "TN_REG" and 136 in (c.Ka, c.Nb),
    "reg_dim60_f32B": lambda c, p: p.route == "TN_REG" and c.Nb == 60 and c.dtB == "f32",
    "reg_dim276_f32A": lambda c, p: p.route == "TN_REG" and c.Ka == 276 and c.dtA == "f32",
    "big": lambda c, p: p.route == "TN_BIG" and p.kernel == "gemm_tn_big_kernel" and c.M == 32768 and not c.brs_T,
    "big_brs_T128": lambda c, p: p.route == "TN_BIG" and c.M == 32768 and c.brs_T == 128,
    "big_off_falls_to_tr": lambda c, p: _tr(c, p) and (c.M, c.Ka, c.Nb, c.nt_big) == (32768, 512, 512, 0),
    "big_off_falls_to_tr_brs": lambda c, p: p.route == "TN_TR_BRS" and (c.M, c.Ka, c.Nb, c.nt_big) == (32768, 512, 512, 0),
}


# ------------------------------------------------------------------ inputs
def round_bf16(x):
    """fp64 / fp32 array -> the nearest bf16 values (ties to even), as fp64"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32).astype(np.float64)


def _store(x, dt):
    return round_bf16(x) if dt == "bf16" else np.asarray(x, np.float32).astype(np.float64)


def has_rs(c):
    return bool(c.brs_T) or c.psa_rs


def rs_T(c):
    return c.brs_T or c.psa_T


def ldw(c):
    return c.Nb + 8          # a weight shadow wider than the GEMM's N


@functools.lru_cache(maxsize=3)
def inputs(name, real):
    """the operands of a case as fp64 arrays holding values of the storage types: A, B, out0, db0 and, where the case has them, rs, P, Q, W"""
    c = BY_NAME[name]
    g = np.random.default_rng(zlib.crc32(name.encode()) * 2 + int(real))
    op = {}
    if real:
        op["A"], op["B"] = _store(g.standard_normal((c.M, c.Ka)), c.dtA), _store(g.standard_normal((c.M, c.Nb)), c.dtB)
    else:
        op["A"], op["B"] = g.integers(-2, 3, (c.M, c.Ka)).astype(np.float64), g.integers(-2, 3, (c.M, c.Nb)).astype(np.float64)
    if c.ka_valid:
        op["A"][:, c.ka_valid:] = 0.0          # zero padding, as the packed stem operand has it
    if c.nb_valid:
        op["B"][:, c.nb_valid:] = 0.0
    kv, nv = c.ka_valid or c.Ka, c.nb_valid or c.Nb
    op["out0"] = np.zeros((kv, nv)) if real else g.integers(-8, 9, (kv, nv)).astype(np.float64)
    op["db0"] = np.zeros(nv) if real else g.integers(-8, 9, nv).astype(np.float64)
    if has_rs(c):
        op["rs"] = g.choice(RS_SET, -(-c.M // rs_T(c)))
        op["rs"][:3] = RS_SET[g.permutation(3)][: len(op["rs"][:3])]          # neighbours that differ, a dropped sample among them
    if c.psa_T:
        Bn = c.M // c.psa_T
        if real:
            op["P"], op["Q"] = _store(g.standard_normal((Bn, c.Ka)), "f32"), _store(g.standard_normal((Bn, c.Ka)), "f32")
            op["W"] = _store(g.standard_normal((c.Ka, ldw(c))), "bf16")
        else:
            op["P"], op["Q"] = g.choice(PQ_SET, (Bn, c.Ka)), g.choice(PQ_SET, (Bn, c.Ka))
            op["W"] = g.integers(-2, 3, (c.Ka, ldw(c))).astype(np.float64)
    return op


# ------------------------------------------------------------------ reference, magnitudes, bounds
def _staged(c, op):
    """A and B as the kernel multiplies them: an f32 operand of a bf16 MFMA is rounded to bf16 while it is staged"""
    A, B = op["A"], op["B"]
    if dtm(c) == "bf16":
        A = round_bf16(A) if c.dtA == "f32" else A
        B = round_bf16(B) if c.dtB == "f32" else B
    return A, B


def _compute(c, A, B, op, absolute, Bsum=None):
    """out, dbias (without the pre-fill), G, Rpart of the operation in fp64; absolute: every factor replaced by its magnitude — the sums of
    absolute values that bound every intermediate and scale the error bound.  Bsum: the B the bias gradient sums (the register-transposing
    kernel takes its column sums from the values it loaded, before an f32 B is rounded to bf16 for the MFMA)"""
    f = np.abs if absolute else (lambda x: x)
    A, B = f(A), f(B)
    Bsum = B if Bsum is None or c.psa_T else f(Bsum)
    kv, nv = c.ka_valid or c.Ka, c.nb_valid or c.Nb
    res = {}
    rows = f(op["rs"])[np.arange(c.M) // rs_T(c)] if has_rs(c) else np.ones(c.M)
    res["dbias"] = (rows[:, None] * Bsum).sum(0)[:nv]
    if c.psa_T:
        Bn, T = c.M // c.psa_T, c.psa_T
        A3, B3 = A.reshape(Bn, T, c.Ka), B.reshape(Bn, T, c.Nb)
        S = np.matmul(A3.transpose(0, 2, 1), B3)                       # [b, k, n]: A_b^T B_b
        g = B3.sum(1)
        res["out"] = (f(op["P"])[:, :, None] * S).sum(0) + np.einsum("bk,bn->kn", f(op["Q"]), g)
        res["G"] = g
        res["Rpart"] = (f(op["W"])[None, :, : c.Nb] * S).reshape(Bn, c.Ka, c.Nb // 64, 64).sum(3).transpose(0, 2, 1)
    else:
        res["out"] = (A.T @ B)[:kv, :nv]
    if not c.bias:
        res.pop("dbias")
    return res


def mutate(c, op, mut, plan=None):
    """the operands with one ordinary mistake applied (test_gemm_tn_mutants.py); returns (A, B, op')"""
    A, B = _staged(c, op)
    op = dict(op)
    assert c.dtB == "bf16"            # (the bias gradient sums the staged B here)
    if mut == "drop_stage":           # the last 32-row stage of one split is never multiplied
        i = plan.splits // 2
        end = min(c.M, (i + 1) * plan.rps)
        A, B = A.copy(), B.copy()
        A[end - 32:end] = 0.0
        B[end - 32:end] = 0.0
    elif mut == "neighbour_scale":    # one sample's bias scale taken from its neighbour
        rs = op["rs"].copy()
        b = next(i for i in range(len(rs) - 1) if rs[i] != rs[i + 1])
        rs[b] = rs[b + 1]
        op["rs"] = rs
    elif mut == "no_q":               # one sample's Q term left out
        Q = op["Q"].copy()
        Q[len(Q) // 2] = 0.0
        op["Q"] = Q
    else:
        raise ValueError(mut)
    return A, B, op


def reference(c, op, mut=None, plan=None):
    """what the call must leave in out, dbias, G, Rpart (fp64)"""
    A, B = _staged(c, op)
    Bsum = op["B"]
    if mut:
        A, B, op = mutate(c, op, mut, plan)
        Bsum = B
    res = _compute(c, A, B, op, False, Bsum)
    res["out"] = res["out"] + op["out0"]
    if "dbias" in res:
        res["dbias"] = res["dbias"] + op["db0"]
    return res


def magnitudes(c, op):
    A, B = _staged(c, op)
    res = _compute(c, A, B, op, True, op["B"])
    res["out"] = res["out"] + np.abs(op["out0"])
    if "dbias" in res:
        res["dbias"] = res["dbias"] + np.abs(op["db0"])
    return res


def bounds(c, op):
    """|err| <= c * M * 2^-24 * magnitude, elementwise: the worst case of fp32 summation in any order.  c = 2 for plain sums, 4 for the per-sample
    fold (out of a PSA call) and Rpart"""
    mag = magnitudes(c, op)
    cc = {"out": 4.0 if c.psa_T else 2.0, "dbias": 2.0, "G": 2.0, "Rpart": 4.0}
    return {n: cc[n] * c.M * U * m for n, m in mag.items()}


@functools.lru_cache(maxsize=3)
def expected(name, real):
    """(reference, bounds or None) of a case on its own inputs; kept for the runs of the case that follow each other"""
    c, op = BY_NAME[name], inputs(name, real)
    return reference(c, op), (bounds(c, op) if real else None)


def worst_ratio(got, ref, bound):
    """name -> max over elements of |got - ref| / bound (0 / 0 counts as 0, x / 0 as inf)"""
    out = {}
    for n in ref:
        err = np.abs(np.asarray(got[n], np.float64) - ref[n])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / bound[n])
        out[n] = float(r.max())
    return out


# ------------------------------------------------------------------ the library: plan and device run
def _fake(i):
    return 4096 * (i + 1)            # a made-up aligned address: the plan entry and a refused call dereference nothing


def make_call(c, ptrs=None):
    """the ishara_gemm_tn_call of a case; ptrs: name -> address (default: made-up aligned addresses for everything the case has)"""
    names = ["A", "B", "out"] + (["dbias"] if c.bias else []) + (["bias_rowscale"] if has_rs(c) else []) + (["P", "Q", "W", "G", "Rpart"] if c.psa_T else [])
    if ptrs is None:
        ptrs = {n: _fake(i) for i, n in enumerate(names)}
    k = _lib.GemmTnCall()
    for n in names:
        setattr(k, n, ptrs[n])
    k.dtA, k.dtB, k.dtM = DT[c.dtA], DT[c.dtB], DT[dtm(c)]
    k.M, k.Ka, k.Nb, k.ka_valid, k.nb_valid = c.M, c.Ka, c.Nb, c.ka_valid, c.nb_valid
    k.bias_T, k.psa_T, k.ldw = (rs_T(c) if has_rs(c) else 0), c.psa_T, (ldw(c) if c.psa_T else 0)
    return k


class switches:
    """the debug switches a case runs under, restored on the way out"""
    def __init__(self, lib, nt_big=1, force=False):
        self.lib, self.nt_big, self.force = lib, nt_big, force

    def __enter__(self):
        self.lib.ishara_debug_set_nt_big(self.nt_big)
        self.lib.ishara_debug_force_regstage(FORCE_TN_REG if self.force else 0)

    def __exit__(self, *a):
        self.lib.ishara_debug_set_nt_big(1)
        self.lib.ishara_debug_force_regstage(0)


def plan(lib, c, force=False):
    """route, profiler key, M-splits and rows per split of the case, from the function the launcher launches from (host only)"""
    route, kernel, splits, rps = C.c_char_p(), C.c_char_p(), C.c_int32(), C.c_int32()
    k = make_call(c)
    with switches(lib, c.nt_big, force):
        rc = lib.ishara_debug_gemm_tn_plan(C.byref(k), C.byref(route), C.byref(kernel), C.byref(splits), C.byref(rps))
    assert rc == 0, lib.ishara_last_error()
    return Plan(route.value.decode(), kernel.value.decode(), splits.value, rps.value)


def slab_bytes(lib, cases):
    arr = (_lib.GemmTnCall * len(cases))(*[make_call(c) for c in cases])
    n = lib.ishara_op_gemm_tn_scratch_bytes(arr, len(cases))
    assert n > 0
    return n


def run(lib, items, deferred, slabs, force=False):
    """runs the calls `items` = [(case, operands)] as one list through ishara_op_gemm_tn (deferred: through one deferred-sum state) and returns,
    per call, the outputs as fp32 arrays plus "guards_ok".  slabs: three device f32 tensors of at least slab_bytes each; what the calls may use
    of them is poisoned with NaN first, so a sum that reads a partial nobody wrote shows"""
    import torch
    dev = slabs[0].device

    def dev_in(x, dt):
        t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
        return (t.to(torch.bfloat16) if dt == "bf16" else t).to(dev)

    def dev_out(x0, shape):
        n = int(np.prod(shape))
        t = torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        if x0 is not None:
            t[:n] = torch.from_numpy(np.ascontiguousarray(x0, np.float32)).reshape(-1).to(dev)
        return t

    need = slab_bytes(lib, [c for c, _ in items])
    assert all(s.dtype == torch.float32 and s.numel() * 4 >= need for s in slabs)
    for s in slabs:
        s[: need // 4].fill_(float("nan"))
    keep, outs, calls = [], [], []
    for c, op in items:
        kv, nv = c.ka_valid or c.Ka, c.nb_valid or c.Nb
        t = {"A": dev_in(op["A"], c.dtA), "B": dev_in(op["B"], c.dtB), "out": dev_out(op["out0"], (kv, nv))}
        shapes = {"out": (kv, nv)}
        if c.bias:
            t["dbias"], shapes["dbias"] = dev_out(op["db0"], (nv,)), (nv,)
        if has_rs(c):
            t["bias_rowscale"] = dev_in(op["rs"], "f32")
        if c.psa_T:
            Bn = c.M // c.psa_T
            t["P"], t["Q"], t["W"] = dev_in(op["P"], "f32"), dev_in(op["Q"], "f32"), dev_in(op["W"], "bf16")
            shapes["G"], shapes["Rpart"] = (Bn, c.Nb), (Bn, c.Nb // 64, c.Ka)
            t["G"], t["Rpart"] = dev_out(None, shapes["G"]), dev_out(None, shapes["Rpart"])
        keep.append(t)
        outs.append(shapes)
        calls.append(make_call(c, {n: v.data_ptr() for n, v in t.items()}))
    arr = (_lib.GemmTnCall * len(calls))(*calls)
    sp = [C.c_void_p(s.data_ptr()) for s in slabs]
    nt_big = {c.nt_big for c, _ in items}
    assert len(nt_big) == 1
    with switches(lib, nt_big.pop(), force):
        rc = lib.ishara_op_gemm_tn(arr, len(calls), sp[0], sp[1] if deferred else None, sp[2] if deferred else None, _lib.stream())
        _lib.check(rc, "ishara_op_gemm_tn")
        torch.cuda.synchronize()
    results = []
    for t, shapes in zip(keep, outs):
        r = {"guards_ok": True}
        for n, shape in shapes.items():
            h = t[n].cpu().numpy()
            k = int(np.prod(shape))
            r[n] = h[:k].reshape(shape)
            r["guards_ok"] = r["guards_ok"] and bool(np.all(h[k:] == np.float32(SENTINEL)))
        results.append(r)
    return results
