"""The three tile kernels of gemm_nt.hip (gemm_nt_t_kernel NT_TILE_T, gemm_nt_glds_kernel NT_GLDS, gemm_nt_kernel NT_REG) through the handle-free
entry ishara_op_gemm_nt against int64 / fp64 numpy: case table, inputs, references, bounds, fingerprint operands and the device runner shared by
test_gemm_nt_plan.py (CPU), test_gemm_nt_mutants.py (CPU) and test_gemm_nt_gpu.py.

Exact form.  Operands and epilogue inputs are small integers in their storage type (A, Wt in [-4, 4], bias / PE table / residual in [-8, 8], the
act' operand in [-2, 2], the column affine's c1 in {-2, -1, 1, 2}), the row scale is one of 1, 2, 4, the dropout rate is 0.5 (scale exactly 2),
act is none or ReLU, dact is DACT_POS.  Every partial sum and every epilogue intermediate is then an integer below 2^24 in magnitude
(test_gemm_nt_plan.py asserts it per case from the sums of absolute values): fp32 gives the same value in any summation order, and the fp64
reference rounded ONCE to dtC (round to nearest even) must be array_equal to C, pre_out, q, k and vt.

Real-valued form.  The same cases with N(0, 1) operands rounded to storage, held to the worst case of fp32 summation in any order:
  |err[m, n]| <= 2 K 2^-24 (|A| |Wt|^T + every epilogue addend's magnitude)[m, n] + u(dtC) |ref[m, n]|,   u = 2^-8 bf16, 2^-11 f16, 2^-24 f32.
Where a kernel rounds the staged operand to the MFMA type (an f32 A under dtM = bf16 / f16, a transformed operand) the reference rounds it the
same way; the column affine keeps c1 a power of two, so v * c1 + c0 is one fp32 rounding whether or not the compiler contracts it.  An f32
transformed operand carries one more fp32 rounding per element, far inside the factor 2 of the bound.  Swish / dSwish cases (real-valued only) use
TOL of test_ops_gpu.py: the fast exponential has no derivable bound here.

Guards and poison.  Every output sits between GUARD sentinel floats that must come back untouched.  Bt rows n >= N are NaN (every kernel computes
and discards those columns); Bt columns k in [K, ldb) are zero — the contract in the head of api_gemm_nt.hip.  The column affine's c1 / c0 are NaN
past K (read by the register-staged kernel on its zero-filled tail and cleared again).

Fingerprint operands (dtC = f32, nk <= 8 K tiles).  "W": A = 1, Wt[n, k] = 8^(k div BK) / BK, so K tile kt contributes exactly one base-8 digit 1;
"A": Wt = 1, A[m, k] = a(m) 8^(k div BK) / BK with a(m) = 1 + (m + m div 128) mod 3.  decode(value, nk) turns an element into its digits: a missing
K tile reads 0, a doubled one 2 a, a stale ring slot puts the digit of kt - 3 (NT_TILE_T) or kt - 4 (NT_GLDS) in place of kt's."""
import ctypes as C
import functools
import zlib
from collections import namedtuple

import numpy as np

from ishara_amd import _lib

DT = {"f32": _lib.F32, "bf16": _lib.BF16, "f16": _lib.F16}
U = 2.0 ** -24
UC = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11}
TOL = {"f32": dict(rtol=2e-4, atol=2e-4), "bf16": dict(rtol=3e-2, atol=3e-2), "f16": dict(rtol=3e-2, atol=3e-2)}     # test_ops_gpu.py's (f16: bf16's, the looser of the 16-bit pair there)
GUARD = 64                    # floats (256 bytes) in front of and behind every output
SENTINEL = {"f32": 77777.0, "bf16": 77824.0, "f16": 60000.0}          # representable in the type, outside every case's value range
GRID = 768                    # run_nt_t: min(ntiles, 768) persistent workgroups
FORCE = {"NT_TILE_T": 8192, "NT_GLDS": 8, "NT_REG": 1}           # ishara_debug_force_regstage
OP = {"none": 0, "swish": 1, "colaffine": 2, "rowscale": 3, "dropmask": 4}
ACT = {"none": 0, "swish": 1, "relu": 2}
DACT = {"none": 0, "swish": 1, "pos": 2}
SEED, OP_SITE, EPI_SITE = 20240, 7, 11

# route: the route the row claims (test_gemm_nt_plan.py holds it to ishara_debug_gemm_nt_route); force: under that route's switch (else the
# default route); tab: the PE table's period (0: none); rowscale: 0 none, 1 on the value, 2 on the bias only; qkv: (H, dh, head_major); T: frames
# per sample of the row scale / QKV split; fp: fingerprint operands "W" / "A"; real_only: Swish somewhere; refused: the entry refuses the call
Case = namedtuple("Case", "name route force M N K dtA dtM dtC op bias tab pre_out act drop rowscale dact resid qkv T fp real_only refused props")


def case(name, route, M, N, K, props, dt="bf16", dtA=None, dtC=None, force=True, op="none", bias=True, tab=0, pre_out=False, act="none", drop=False,
         rowscale=0, dact="none", resid=False, qkv=None, T=0, fp=None, refused=False):
    real_only = "swish" in (op, act, dact)
    if fp:
        bias = False
    return Case(name, route, force, M, N, K, dtA or dt, dt, dtC or dt, op, bias, tab, pre_out, act, drop, rowscale, dact, resid, qkv, T, fp, real_only,
                refused, tuple(props.split()))


def _epilogues(p, route, dt="bf16"):
    """the generic-epilogue list of the 128 x 128 and 64 x 128 kernels on small two-row-tile shapes"""
    return [
        case(f"{p}_addtab", route, 200, 132, 64, f"{p}_addtab", dt, tab=72),
        case(f"{p}_preout_relu", route, 130, 64, 64, f"{p}_preout_relu", dt, pre_out=True, act="relu"),
        case(f"{p}_drop", route, 130, 68, 64, f"{p}_drop", dt, drop=True),
        case(f"{p}_rowscale0", route, 192, 64, 64, f"{p}_rowscale0", dt, rowscale=1, T=24),
        case(f"{p}_rowscale1", route, 192, 64, 64, f"{p}_rowscale1", dt, rowscale=2, T=24),
        case(f"{p}_dact", route, 130, 60, 64, f"{p}_dact", dt, dact="pos"),
        case(f"{p}_dact_resid", route, 130, 124, 64, f"{p}_dact_resid", dt, dact="pos", resid=True),
        case(f"{p}_qkv_hm1", route, 6 * 24, 48, 64, f"{p}_qkv_hm1", dt, qkv=(2, 8, 1), T=24),
        case(f"{p}_qkv_hm0", route, 4 * 40, 192, 64, f"{p}_qkv_hm0", dt, qkv=(2, 32, 0), T=40),
        case(f"{p}_swish", route, 130, 64, 64, f"{p}_swish", dt, pre_out=True, act="swish"),
        case(f"{p}_dswish", route, 130, 64, 64, f"{p}_dswish", dt, dact="swish", resid=True),
    ]


T_, G_, R_ = "NT_TILE_T", "NT_GLDS", "NT_REG"
CASES = [
    # ---- NT_TILE_T: K tiles (bf16 32, f32 16): the prologue's st < nk, the vmcnt(4) / vmcnt(0) choice, kt + 2 < nk
    *[case(f"t_nk{n}", T_, 128, 128, 32 * n, f"t_nk{n} t_bf16", resid=n % 2 == 0) for n in (1, 2, 3, 4, 5, 6, 7)],
    case("t_nk20", T_, 256, 128, 640, "t_nk20 t_ek2", resid=True),
    *[case(f"t_f32_nk{n}", T_, 130, 64, 16 * n, f"t_nk{n} t_f32", "f32") for n in (1, 3, 4)],
    # ---- M edges (clamped A rows, mrow + 16 i >= M) with N edges on one and on two column tiles
    case("t_m256_n4", T_, 256, 4, 64, "t_mmod0 t_nmod4_1 t_ek1"),
    case("t_m129_n60", T_, 129, 60, 64, "t_mmod1 t_nmod60_1 t_ek2", resid=True),
    case("t_m143_n64", T_, 143, 64, 64, "t_mmod15 t_nmod64_1", "f32"),
    case("t_m16_n68", T_, 16, 68, 64, "t_mmod16 t_nmod68_1", resid=True),
    case("t_m145_n124", T_, 145, 124, 64, "t_mmod17 t_nmod124_1", dtC="f32"),
    case("t_m191_n132", T_, 191, 132, 64, "t_mmod63 t_nmod4_2", resid=True),
    case("t_m64_n188", T_, 64, 188, 64, "t_mmod64 t_nmod60_2", "f32", resid=True),
    case("t_m193_n192", T_, 193, 192, 64, "t_mmod65 t_nmod64_2 t_bf16_f32", dtC="f32", resid=True),
    case("t_m255_n196", T_, 255, 196, 64, "t_mmod127 t_nmod68_2"),
    case("t_m130_n252", T_, 130, 252, 64, "t_nmod124_2", resid=True),
    # ---- tile mapping: 8 row tiles (XCD-aware) and 3 (plain), three column tiles
    case("t_xcd", T_, 8 * 128, 260, 96, "t_xcd", resid=True),
    case("t_noxcd", T_, 3 * 128 - 5, 260, 96, "t_noxcd"),
    # ---- persistent rounds: more than 768 tiles
    case("t_p769_row1", T_, 98305, 128, 32, "t_p769_row1 t_pnk1", resid=True),
    case("t_p769", T_, 98432, 128, 64, "t_p769 t_pnk2"),
    case("t_p1538", T_, 98432, 256, 64, "t_p1538"),
    case("t_p776_xcd", T_, 99328, 128, 64, "t_p776_xcd", resid=True),
    case("t_p770_ragged", T_, 49153, 132, 64, "t_p770_ragged", resid=True),
    case("t_p769_nk3", T_, 98432, 128, 96, "t_pnk3", resid=True),
    case("t_p769_nk4", T_, 98432, 128, 128, "t_pnk4"),
    case("t_p769_relu", T_, 98432, 128, 32, "t_pek0_relu", act="relu"),
    case("t_reported", T_, 34816, 768, 640, "t_reported", resid=True),
    # ---- the generic epilogue (EK 0), dtypes, fingerprints
    *_epilogues("t", T_),
    case("t_f32_dact_resid", T_, 130, 124, 48, "t_f32_epi", "f32", dact="pos", resid=True),
    case("t_bf16_f32_qkv", T_, 6 * 24, 48, 64, "t_bf16_f32_epi", dtC="f32", qkv=(2, 8, 1), T=24),
    case("t_fpW", T_, 130, 132, 256, "t_fpW_single", dtC="f32", fp="W"),
    case("t_fpA", T_, 130, 132, 256, "t_fpA_single", dtC="f32", fp="A"),
    case("t_fpW_f32", T_, 128, 128, 112, "t_fp_f32", "f32", fp="W"),
    case("t_fpW_p769", T_, 98432, 128, 128, "t_fpW_769", dtC="f32", fp="W"),
    case("t_fpA_p769", T_, 98305, 128, 96, "t_fpA_769", dtC="f32", fp="A"),
    case("t_default", T_, 130, 132, 64, "t_default_route", force=False, resid=True),
    # ---- NT_GLDS: ring of 4 (nk 1 .. 9: wraps at 4, ahead 2 / 1 / 0), M mod 64, N, tile mapping
    *[case(f"g_nk{n}", G_, 64, 128, 32 * n, f"g_nk{n} g_bf16", resid=n % 2 == 1) for n in range(1, 10)],
    *[case(f"g_f32_nk{n}", G_, 70, 64, 16 * n, f"g_nk{n} g_f32", "f32") for n in (2, 5, 9)],
    case("g_m128_n8", G_, 128, 8, 64, "g_mmod0 g_n8"),
    case("g_m65_n60", G_, 65, 60, 64, "g_mmod1 g_n60", resid=True),
    case("g_m71_n64", G_, 71, 64, 64, "g_mmod7 g_n64", "f32", resid=True),
    case("g_m8_n124", G_, 8, 124, 64, "g_mmod8 g_n124"),
    case("g_m73_n132", G_, 73, 132, 64, "g_mmod9 g_n132 g_bf16_f32", dtC="f32", resid=True),
    case("g_m95_n60", G_, 95, 60, 64, "g_mmod31", "f32"),
    case("g_m32_n132", G_, 32, 132, 64, "g_mmod32", resid=True),
    case("g_m97_n8", G_, 97, 8, 64, "g_mmod33", resid=True),
    case("g_m127_n124", G_, 127, 124, 64, "g_mmod63", dtC="f32"),
    case("g_xcd", G_, 8 * 64, 132, 160, "g_xcd", resid=True),
    case("g_noxcd", G_, 5 * 64 - 3, 132, 160, "g_noxcd"),
    case("g_default_n62", G_, 70, 62, 64, "g_default_route", force=False, resid=True),
    *_epilogues("g", G_),
    case("g_f32_rowscale", G_, 192, 64, 48, "g_f32_epi", "f32", rowscale=2, T=24, pre_out=True, act="relu"),
    case("g_fpW", G_, 70, 132, 256, "g_fpW", dtC="f32", fp="W"),
    case("g_fpA", G_, 70, 132, 256, "g_fpA", dtC="f32", fp="A"),
    case("g_fpA_f32", G_, 130, 64, 128, "g_fp_f32", "f32", fp="A"),
    # ---- NT_REG: K tiles of 64 bf16 / 32 f32, ragged K, operand transforms, mixed types, fp16
    case("r_k8", R_, 129, 8, 8, "r_nk1 r_K8 r_mmod1 r_n8", force=False),
    case("r_k72", R_, 191, 60, 72, "r_nk2 r_K72 r_mmod63 r_n60", force=False, resid=True),
    case("r_k136", R_, 64, 130, 136, "r_nk3 r_K136 r_mmod64 r_n130", force=False),
    case("r_f32_k4", R_, 193, 8, 4, "r_K4 r_mmod65", "f32", force=False, resid=True),
    case("r_f32_k36", R_, 255, 60, 36, "r_K36 r_mmod127", "f32", force=False),
    case("r_f32_k276", R_, 130, 130, 276, "r_K276", "f32", force=False, resid=True),
    case("r_forced", R_, 130, 132, 128, "r_forced_whole_tiles", resid=True),
    case("r_forced_f32", R_, 130, 64, 96, "r_forced_whole_tiles_f32", "f32", pre_out=True, act="relu"),
    case("r_colaffine_f32", R_, 130, 60, 36, "r_colaffine_f32", "f32", force=False, op="colaffine"),
    case("r_colaffine_bf16", R_, 130, 60, 136, "r_colaffine_bf16", force=False, op="colaffine", resid=True),
    case("r_dropmask_f32", R_, 130, 60, 36, "r_dropmask_f32", "f32", force=False, op="dropmask", dact="pos"),
    case("r_dropmask_bf16", R_, 130, 130, 72, "r_dropmask_bf16", force=False, op="dropmask"),
    case("r_swish_f32", R_, 130, 60, 36, "r_swish_f32", "f32", force=False, op="swish"),
    case("r_swish_bf16", R_, 130, 60, 72, "r_swish_bf16", force=False, op="swish"),
    case("r_f32_bf16_bf16", R_, 130, 60, 72, "r_f32_bf16_bf16", dtA="f32", force=False, resid=True),
    case("r_bf16_bf16_f32", R_, 130, 130, 72, "r_bf16_bf16_f32", dtC="f32", force=True, resid=True),
    case("r_f16", R_, 130, 60, 72, "r_f16_f16_f16", "f16", force=False, resid=True),
    case("r_f16_f32", R_, 129, 130, 136, "r_f16_f16_f32", "f16", dtC="f32", force=False),
    case("r_f32_f16", R_, 130, 60, 72, "r_f32_f16_f16", "f16", dtA="f32", force=False, act="relu"),
    case("r_qkv_hm1", R_, 6 * 24, 48, 72, "r_qkv_hm1", force=False, qkv=(2, 8, 1), T=24),
    case("r_qkv_hm0", R_, 4 * 40, 192, 72, "r_qkv_hm0", force=False, qkv=(2, 32, 0), T=40),
    case("r_addtab_drop", R_, 200, 60, 72, "r_addtab_drop", force=False, tab=72, drop=True),
    # ---- refused rows.  a_vec_ok = false (A rows off 16 bytes) cannot reach gemm_nt_kernel: launch_gemm_nt refuses K % 8 (16-bit) / K % 4 first
    case("r_refused_rowscale", R_, 130, 60, 72, "r_refused_op_rowscale", force=False, op="rowscale", refused=True),
    case("r_refused_f16_op", R_, 130, 60, 72, "r_refused_f16_op", "f16", force=False, op="dropmask", refused=True),
    case("r_refused_avec_bf16", R_, 130, 60, 12, "r_refused_avec_false", force=False, refused=True),
    case("r_refused_avec_f32", R_, 130, 60, 6, "r_refused_avec_false", "f32", force=False, refused=True),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RUN_CASES = [c for c in CASES if not c.refused]
EXACT_CASES = [c for c in RUN_CASES if not c.real_only]
# the persistent and fingerprint cases of NT_TILE_T: run five times into five fresh output buffers
REPEAT_CASES = [c for c in EXACT_CASES if c.route == T_ and (c.fp or -(-c.M // 128) * -(-c.N // 128) > GRID)]
REPORTED = "t_reported"


# ------------------------------------------------------------------ geometry, computed from the shape and the route's tile sizes
def bm(c):
    return 64 if c.route == G_ else 128


def bk(c):
    """the route's K tile: LDS-DMA kernels 32 (16-bit) / 16 (f32), the register-staged kernel 64 / 32"""
    return (2 if c.route == R_ else 1) * (16 if c.dtM == "f32" else 32)


def nk(c):
    return -(-c.K // bk(c))


def n_mt(c):
    return -(-c.M // bm(c))


def n_nt(c):
    return -(-c.N // 128)


def ntiles(c):
    return n_mt(c) * n_nt(c)


def grid(c):
    return min(ntiles(c), GRID) if c.route == T_ else ntiles(c)


def ring(c):
    return {T_: 3, G_: 4, R_: 2}[c.route]


def tile_id(c, mt, nt):
    """the inverse of the kernels' tile_of: XCD-aware when the row-tile count is a multiple of 8"""
    if n_mt(c) % 8 == 0:
        return ((mt // 8) * n_nt(c) + nt) * 8 + mt % 8
    return mt * n_nt(c) + nt


def tile_of(c, tid):
    if n_mt(c) % 8 == 0:
        xcd, local = tid & 7, tid >> 3
        return (local // n_nt(c)) * 8 + xcd, local % n_nt(c)
    return tid // n_nt(c), tid % n_nt(c)


def ldb(c):
    return -(-c.K // 64) * 64 if c.dtM != "f32" else -(-c.K // 32) * 32


def bt_rows(c):
    return n_nt(c) * 128


def ek(c):
    """the epilogue variant run_nt_t picks"""
    fast = not (c.tab or c.pre_out or c.act != "none" or c.drop or c.rowscale or c.dact != "none" or c.qkv)
    return (2 if c.resid else 1) if fast else 0


def _epi(c, **kw):
    return c.route in (T_, G_) and ek(c) == 0 and all(getattr(c, k) == v for k, v in kw.items())


def _route_props(p, route):
    return {
        f"{p}_addtab": lambda c: _epi(c, route=route) and 0 < c.tab < c.M and 128 % c.tab != 0 and c.tab % 128 != 0,
        f"{p}_preout_relu": lambda c: _epi(c, route=route, pre_out=True, act="relu"),
        f"{p}_drop": lambda c: _epi(c, route=route, drop=True),
        f"{p}_rowscale0": lambda c: _epi(c, route=route, rowscale=1) and c.T % 128 != 0 and c.bias,
        f"{p}_rowscale1": lambda c: _epi(c, route=route, rowscale=2) and c.T % 128 != 0 and c.bias,
        f"{p}_dact": lambda c: _epi(c, route=route, dact="pos", resid=False),
        f"{p}_dact_resid": lambda c: _epi(c, route=route, dact="pos", resid=True),
        f"{p}_qkv_hm1": lambda c: c.route == route and c.qkv and c.qkv[1:] == (8, 1) and c.T % 8 == 0 and c.T % 128 != 0,
        f"{p}_qkv_hm0": lambda c: c.route == route and c.qkv and c.qkv[1:] == (32, 0) and c.T % 8 == 0 and c.T % 128 != 0,
        f"{p}_swish": lambda c: _epi(c, route=route, act="swish", pre_out=True),
        f"{p}_dswish": lambda c: _epi(c, route=route, dact="swish"),
    }


def _t(c):
    return c.route == T_


def _pers(c, tiles=None):
    return _t(c) and c.K in (32, 64, 96, 128) and c.N <= 256 and (tiles is None or ntiles(c) == tiles)


def _dts(c, a, m, cc):
    return (c.dtA, c.dtM, c.dtC) == (a, m, cc)


# property -> predicate over the case, computed from M, N, K, the route's tile and K-tile sizes and the 768-workgroup grid; every property needs
# a case, every case keeps its own (test_gemm_nt_plan.py)
PROPS = {
    **{f"t_nk{n}": (lambda c, n=n: _t(c) and nk(c) == n and c.K % bk(c) == 0) for n in (1, 2, 3, 4, 5, 6, 7)},
    "t_nk20": lambda c: _t(c) and nk(c) == 20 and c.K == 640 and c.dtM == "bf16",
    **{f"t_mmod{r}": (lambda c, r=r: _t(c) and c.M % 128 == r) for r in (0, 1, 15, 16, 17, 63, 64, 65, 127)},
    **{f"t_nmod{r}_{k}": (lambda c, r=r, k=k: _t(c) and c.N % 128 == r and n_nt(c) == k and c.bias) for r in (4, 60, 64, 68, 124) for k in (1, 2)},
    "t_xcd": lambda c: _t(c) and n_mt(c) % 8 == 0 and n_nt(c) > 2 and ntiles(c) <= GRID,
    "t_noxcd": lambda c: _t(c) and n_mt(c) % 8 != 0 and n_mt(c) > 1 and n_nt(c) > 2,
    "t_p769_row1": lambda c: _pers(c, 769) and c.M == 768 * 128 + 1 and tile_of(c, GRID) == (768, 0),
    "t_p769": lambda c: _pers(c, 769) and c.M == 769 * 128 and c.N == 128,
    "t_p1538": lambda c: _pers(c, 1538) and -(-ntiles(c) // GRID) == 3 and ntiles(c) - 2 * GRID == 2,
    "t_p776_xcd": lambda c: _pers(c, 776) and n_mt(c) % 8 == 0 and c.N == 128,
    "t_p770_ragged": lambda c: _pers(c, 770) and c.M % 128 == 1 and c.N % 128 == 4,
    **{f"t_pnk{n}": (lambda c, n=n: _pers(c) and ntiles(c) > GRID and nk(c) == n) for n in (1, 2, 3, 4)},
    "t_pek0_relu": lambda c: _pers(c) and ntiles(c) > GRID and ek(c) == 0 and c.act == "relu",
    "t_reported": lambda c: _t(c) and (c.M, c.N, c.K) == (34816, 768, 640) and ek(c) == 2 and _dts(c, "bf16", "bf16", "bf16") and ntiles(c) == 1632,
    "t_ek1": lambda c: _t(c) and ek(c) == 1 and c.bias,
    "t_ek2": lambda c: _t(c) and ek(c) == 2 and c.bias,
    **_route_props("t", T_),
    "t_f32": lambda c: _t(c) and _dts(c, "f32", "f32", "f32"),
    "t_bf16": lambda c: _t(c) and _dts(c, "bf16", "bf16", "bf16"),
    "t_bf16_f32": lambda c: _t(c) and _dts(c, "bf16", "bf16", "f32") and not c.fp,
    "t_f32_epi": lambda c: _epi(c, route=T_) and _dts(c, "f32", "f32", "f32"),
    "t_bf16_f32_epi": lambda c: _t(c) and ek(c) == 0 and _dts(c, "bf16", "bf16", "f32"),
    "t_fpW_single": lambda c: _t(c) and c.fp == "W" and nk(c) == 8 and c.dtM == "bf16" and ntiles(c) <= GRID,
    "t_fpA_single": lambda c: _t(c) and c.fp == "A" and nk(c) == 8 and c.dtM == "bf16" and ntiles(c) <= GRID,
    "t_fp_f32": lambda c: _t(c) and c.fp and c.dtM == "f32" and nk(c) > 3 and ntiles(c) == 1,
    "t_fpW_769": lambda c: _pers(c, 769) and c.fp == "W" and nk(c) > 3,
    "t_fpA_769": lambda c: _pers(c, 769) and c.fp == "A" and nk(c) == 3,
    "t_default_route": lambda c: _t(c) and not c.force,
    **{f"g_nk{n}": (lambda c, n=n: c.route == G_ and nk(c) == n) for n in range(1, 10)},
    **{f"g_mmod{r}": (lambda c, r=r: c.route == G_ and c.M % 64 == r) for r in (0, 1, 7, 8, 9, 31, 32, 33, 63)},
    **{f"g_n{n}": (lambda c, n=n: c.route == G_ and c.N == n and c.bias) for n in (8, 60, 64, 124, 132)},
    "g_xcd": lambda c: c.route == G_ and n_mt(c) % 8 == 0 and n_nt(c) > 1,
    "g_noxcd": lambda c: c.route == G_ and n_mt(c) % 8 != 0 and n_mt(c) > 1 and n_nt(c) > 1,
    "g_default_route": lambda c: c.route == G_ and not c.force and c.N % 4 != 0,
    **_route_props("g", G_),
    "g_f32": lambda c: c.route == G_ and _dts(c, "f32", "f32", "f32"),
    "g_bf16": lambda c: c.route == G_ and _dts(c, "bf16", "bf16", "bf16"),
    "g_bf16_f32": lambda c: c.route == G_ and _dts(c, "bf16", "bf16", "f32") and not c.fp,
    "g_f32_epi": lambda c: _epi(c, route=G_) and _dts(c, "f32", "f32", "f32"),
    "g_fpW": lambda c: c.route == G_ and c.fp == "W" and nk(c) == 8,
    "g_fpA": lambda c: c.route == G_ and c.fp == "A" and nk(c) == 8,
    "g_fp_f32": lambda c: c.route == G_ and c.fp and c.dtM == "f32" and nk(c) > 4,
    **{f"r_nk{n}": (lambda c, n=n: c.route == R_ and nk(c) == n) for n in (1, 2, 3)},
    **{f"r_K{k}": (lambda c, k=k: c.route == R_ and c.K == k and c.K % bk(c) != 0 and c.dtA == ("f32" if k in (4, 36, 276) else "bf16") and not c.force)
       for k in (4, 36, 276, 8, 72, 136)},
    **{f"r_mmod{r}": (lambda c, r=r: c.route == R_ and c.M % 128 == r) for r in (1, 63, 64, 65, 127)},
    **{f"r_n{n}": (lambda c, n=n: c.route == R_ and c.N == n and c.bias) for n in (8, 60, 130)},
    "r_forced_whole_tiles": lambda c: c.route == R_ and c.force and c.K % bk(c) == 0 and c.dtM == "bf16",
    "r_forced_whole_tiles_f32": lambda c: c.route == R_ and c.force and c.K % bk(c) == 0 and c.dtM == "f32",
    **{f"r_{o}_{d}": (lambda c, o=o, d=d: c.route == R_ and c.op == o and _dts(c, d, d, d) and c.K % bk(c) != 0) for o in ("colaffine", "dropmask", "swish") for d in ("f32", "bf16")},
    "r_f32_bf16_bf16": lambda c: c.route == R_ and _dts(c, "f32", "bf16", "bf16"),
    "r_bf16_bf16_f32": lambda c: c.route == R_ and _dts(c, "bf16", "bf16", "f32"),
    "r_f16_f16_f16": lambda c: c.route == R_ and _dts(c, "f16", "f16", "f16"),
    "r_f16_f16_f32": lambda c: c.route == R_ and _dts(c, "f16", "f16", "f32"),
    "r_f32_f16_f16": lambda c: c.route == R_ and _dts(c, "f32", "f16", "f16"),
    "r_qkv_hm1": lambda c: c.route == R_ and c.qkv and c.qkv[2] == 1,
    "r_qkv_hm0": lambda c: c.route == R_ and c.qkv and c.qkv[2] == 0,
    "r_addtab_drop": lambda c: c.route == R_ and c.tab and c.drop and c.N % 8 != 0,
    "r_refused_op_rowscale": lambda c: c.refused and c.op == "rowscale",
    "r_refused_f16_op": lambda c: c.refused and c.dtM == "f16" and c.op != "none",
    "r_refused_avec_false": lambda c: c.refused and (c.K * (4 if c.dtA == "f32" else 2)) % 16 != 0,
}


# ------------------------------------------------------------------ number formats
def round_bf16(x):
    """fp64 / fp32 array -> the nearest bf16 values (ties to even), as fp64"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return b.view(np.float32).astype(np.float64)


def store(x, dt):
    """fp64 array -> the nearest values of the storage type, as fp64 (inputs here are exact in fp32 or N(0, 1) draws: one rounding that matters)"""
    if dt == "bf16":
        return round_bf16(x)
    if dt == "f16":
        return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def decode(value, n):
    """the n base-8 digits of a fingerprint element, K tile 0 first; None for a value that is no non-negative integer below 8^n"""
    if not np.isfinite(value) or value < 0 or value != int(value) or value >= 8 ** n:
        return None
    v = int(value)
    return [(v >> (3 * kt)) & 7 for kt in range(n)]


def fp_row_factor(m):
    m = np.asarray(m)
    return 1 + (m + m // 128) % 3


# ------------------------------------------------------------------ inputs
def qkv_dims(c):
    H, dh, hm = c.qkv
    return c.M // c.T, H, dh, hm


@functools.lru_cache(maxsize=2)
def inputs(name, real):
    """the operands of a case as fp64 arrays holding values of the storage types: A [M, K], W [N, K] and whatever the epilogue reads"""
    c = BY_NAME[name]
    g = np.random.default_rng(zlib.crc32(name.encode()) * 2 + int(real))
    op = {}

    def draw(shape, lo, hi, dt):
        return store(g.standard_normal(shape), dt) if real else g.integers(lo, hi + 1, shape).astype(np.float64)

    if c.fp:
        digit = 8.0 ** (np.arange(c.K) // bk(c)) / bk(c)
        op["A"] = np.ones((c.M, c.K)) if c.fp == "W" else fp_row_factor(np.arange(c.M))[:, None] * digit[None, :]
        op["W"] = np.ones((c.N, c.K)) if c.fp == "A" else np.broadcast_to(digit, (c.N, c.K)).copy()
        return op
    op["A"], op["W"] = draw((c.M, c.K), -4, 4, c.dtA), draw((c.N, c.K), -4, 4, c.dtM)
    if c.bias:
        op["bias"] = draw(c.N, -8, 8, "f32")
    if c.tab:
        op["addtab"] = draw((c.tab, c.N), -8, 8, "f32")
    if c.rowscale:
        op["rowscale"] = g.choice([1.0, 2.0, 4.0], -(-c.M // c.T))
        op["rowscale"][:3] = g.permutation([1.0, 2.0, 4.0])[: len(op["rowscale"][:3])]          # neighbours that differ
    if c.dact != "none":
        op["aux"] = draw((c.M, c.N), -2, 2, c.dtC)
    if c.resid:
        op["resid"] = draw((c.M, c.N), -8, 8, c.dtC)
    if c.op == "colaffine":
        op["c1"] = g.choice([-2.0, -1.0, 1.0, 2.0], c.K)          # powers of two in both forms (see the head of the file)
        op["c0"] = draw(c.K, -2, 2, "f32")
    return op


def cpu_masks(c):
    """the dropout masks of the case (0 or 2) from the oracle's mirror of the device generator — the CPU tests; the GPU tests take them from
    ishara_dropout_mask (device_masks)"""
    from oracle import rng
    m = {}
    if c.op == "dropmask":
        m["op"] = rng.scaled_mask(SEED, OP_SITE, c.M, c.K, 0.5).astype(np.float64)
    if c.drop:
        m["epi"] = rng.scaled_mask(SEED, EPI_SITE, c.M, c.N, 0.5).astype(np.float64)
    return m


# ------------------------------------------------------------------ reference, magnitudes, bounds, mutants
MUTANTS = ["drop_last_ktile", "stale_slot", "clamp_off_by_one", "bias_guard_tile", "resid_neighbour_group", "second_tile_first_coords",
           "rowscale_modes_swapped", "dact_after_resid", "qkv_layouts_swapped", "vt_not_transposed"]


def mutant_applies(c, mut):
    return {
        "drop_last_ktile": nk(c) > 1,
        "stale_slot": nk(c) > ring(c) and c.route != R_,
        "clamp_off_by_one": c.M % bm(c) != 0 and c.M > 1,
        "bias_guard_tile": c.bias and c.N % 128 != 0,
        "resid_neighbour_group": c.resid and c.M > 16,
        "second_tile_first_coords": c.route == T_ and ntiles(c) > GRID,
        "rowscale_modes_swapped": bool(c.rowscale) and c.bias,
        "dact_after_resid": c.dact != "none" and c.resid,
        "qkv_layouts_swapped": bool(c.qkv),
        "vt_not_transposed": bool(c.qkv),
    }[mut]


def staged(c, op, masks, absolute=False):
    """A as the kernel multiplies it: transformed in fp32, rounded to the MFMA type"""
    A = op["A"]
    if c.op == "swish":
        A = A / (1.0 + np.exp(-A))
    elif c.op == "colaffine":
        A = (A * op["c1"][None, :] + op["c0"][None, :]).astype(np.float32).astype(np.float64)
    elif c.op == "dropmask":
        A = A * masks["op"]
    A = store(A, c.dtM)
    return np.abs(A) if absolute else A


def _scatter(c, v):
    """C [M, N] -> q, k [B, H, T, dh], vt [B, H, dh, T]"""
    B, H, dh, hm = qkv_dims(c)
    x = v.reshape(B, c.T, H, 3, dh) if hm else v.reshape(B, c.T, 3, H, dh).transpose(0, 1, 3, 2, 4)
    q, k, vv = (x[:, :, :, i, :].transpose(0, 2, 1, 3) for i in range(3))       # [B, H, T, dh]
    return q, k, vv


def compute(c, op, masks, absolute=False, mut=None):
    """the outputs of the call in fp64, before the rounding to dtC: C (or q, k, vt) and pre_out.  absolute: every factor and addend replaced by its
    magnitude and every gate (ReLU, act') open — the sums that bound every intermediate and scale the error bound.  mut: one ordinary mistake"""
    f = np.abs if absolute else (lambda x: x)
    A, W = staged(c, op, masks, absolute), f(op["W"])
    BK, M, N = bk(c), c.M, c.N
    if mut == "drop_last_ktile":
        A = A.copy()
        A[:, (nk(c) - 1) * BK:] = 0.0
    acc = A @ W.T
    if mut == "stale_slot":            # one output tile multiplies, at K tile kt, what the ring slot held a lap earlier
        kt, kold = nk(c) - 1, nk(c) - 1 - ring(c)
        mt, nt = tile_of(c, ntiles(c) - 1)
        rs_, cs_ = slice(mt * bm(c), min(M, (mt + 1) * bm(c))), slice(nt * 128, min(N, (nt + 1) * 128))
        new, old = slice(kt * BK, (kt + 1) * BK), slice(kold * BK, (kold + 1) * BK)
        acc[rs_, cs_] += A[rs_, old] @ W[cs_, old].T - A[rs_, new] @ W[cs_, new].T
    if mut == "clamp_off_by_one":      # rows clamped to M - 2: the last row multiplies its neighbour's
        acc[M - 1] = acc[M - 2]
    if mut == "second_tile_first_coords":      # a workgroup's second tile is computed at its first tile's (mt, nt)
        for tid in range(GRID, min(ntiles(c), 2 * GRID)):
            (mt, nt), (m1, n1) = tile_of(c, tid), tile_of(c, tid - GRID)
            r = min(M, (mt + 1) * 128) - mt * 128
            w = min(N, (nt + 1) * 128) - nt * 128
            acc[mt * 128:mt * 128 + r, nt * 128:nt * 128 + w] = A[m1 * 128:m1 * 128 + r] @ W[n1 * 128:n1 * 128 + w].T
    rows = np.arange(M)
    rsb = c.rowscale == 2
    if mut == "rowscale_modes_swapped" and c.rowscale:
        rsb = not rsb
    rs = f(op["rowscale"])[rows // c.T][:, None] if c.rowscale else None
    v = acc
    if c.bias:
        b = np.broadcast_to(f(op["bias"])[None, :], (M, N)).copy()
        if mut == "bias_guard_tile":
            b[:, (N // 128) * 128:] = 0.0
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
    res = None
    if c.resid:
        res = f(op["resid"])
        if mut == "resid_neighbour_group":      # rows 0..15 take the residual of rows 16..31
            res = res.copy()
            res[:16] = res[16:32] if M >= 32 else np.roll(res[:32], -16, 0)[:16]
    if mut == "dact_after_resid" and res is not None:
        v, res = v + res, None
    if c.dact == "pos" and not absolute:
        v = np.where(op["aux"] > 0, v, 0.0)
    elif c.dact == "swish":
        a = op["aux"]
        s = 1.0 / (1.0 + np.exp(-a))
        v = v * (np.abs(s * (1.0 + a * (1.0 - s))) if absolute else s * (1.0 + a * (1.0 - s)))
    if res is not None:
        v = v + res
    if not c.qkv:
        out["C"] = v
        return out
    B, H, dh, hm = qkv_dims(c)
    cc = c._replace(qkv=(H, dh, 1 - hm)) if mut == "qkv_layouts_swapped" else c
    q, k, vv = _scatter(cc, v)
    out["q"], out["k"] = np.ascontiguousarray(q), np.ascontiguousarray(k)
    out["vt"] = np.ascontiguousarray(vv).reshape(B, H, dh, c.T) if mut == "vt_not_transposed" else np.ascontiguousarray(vv.transpose(0, 1, 3, 2))
    return out


def reference(c, op, masks, mut=None, rounded=True):
    """what the call must leave in C / q, k, vt and pre_out: fp64, rounded once to dtC (exact form: the comparison is array_equal)"""
    out = compute(c, op, masks, False, mut)
    return {n: store(v, c.dtC) for n, v in out.items()} if rounded else out


def magnitudes(c, op, masks):
    return compute(c, op, masks, True)


def bounds(c, op, masks):
    """elementwise: 2 K 2^-24 * magnitude + u(dtC) * |ref| (see the head of the file)"""
    ref, mag = reference(c, op, masks, rounded=False), magnitudes(c, op, masks)
    return {n: 2.0 * c.K * U * mag[n] + UC[c.dtC] * np.abs(ref[n]) for n in ref}


def worst_ratio(c, got, ref, bound):
    """name -> max over elements of |got - ref| / bound (0 / 0 counts as 0); a Swish case: |got - ref| / (atol + rtol |ref|) with TOL"""
    out = {}
    for n in ref:
        err = np.abs(np.asarray(got[n], np.float64) - ref[n])
        b = TOL[c.dtC]["atol"] + TOL[c.dtC]["rtol"] * np.abs(ref[n]) if c.real_only else bound[n]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0, 0.0, err / b)
        out[n] = float(np.nan_to_num(r, nan=np.inf).max())
    return out


@functools.lru_cache(maxsize=2)
def expected(name, real):
    """(reference, bounds or None) of a case on its own inputs with the oracle's masks; kept for the runs of the case that follow each other.  The
    real-valued reference is not rounded to dtC: the bound carries that rounding"""
    c, op = BY_NAME[name], inputs(name, real)
    m = cpu_masks(c)
    return reference(c, op, m, rounded=not real), (bounds(c, op, m) if real else None)


def describe_wrong(c, name, got, want, limit=6):
    """the first wrong elements of output `name` of an exact case: (m, n), the output tile, for NT_TILE_T the tile id under tile_of's mapping with
    workgroup = id mod grid and round = id div grid, got, want and, for a fingerprint case, the decoded K-tile digits"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    box = " x ".join(f"{int(lo)}..{int(hi)}" for lo, hi in zip(bad.min(0), bad.max(0)))
    lines = [f"{c.name} {name}: {len(bad)} wrong elements of {np.asarray(want).size}, all inside index box {box}"]
    for idx in bad[:limit]:
        idx = tuple(int(i) for i in idx)
        g, w = float(got[idx]), float(want[idx])
        if name in ("C", "pre_out"):
            m, n = idx
        else:      # q, k [B, H, T, dh]; vt [B, H, dh, T]: back to the GEMM's row and column
            B, H, dh, hm = qkv_dims(c)
            b, h, t, i = idx if name != "vt" else (idx[0], idx[1], idx[3], idx[2])
            part = ("q", "k", "vt").index(name)
            m, n = b * c.T + t, (h * 3 * dh + part * dh + i) if hm else (part * H * dh + h * dh + i)
        mt, nt = m // bm(c), n // 128
        s = f"  ({m}, {n}) tile ({mt}, {nt})"
        if c.route == T_:
            tid = tile_id(c, mt, nt)
            s += f" id {tid} workgroup {tid % grid(c)} round {tid // grid(c)}"
            mi, ni = m % 128, n % 128      # the accumulator that holds it: wave (wr, wc), acc[j][i][e] in the lanes of group g = lane >> 4
            s += f" wave ({mi // 64}, {ni // 64}) acc[{ni % 64 // 16}][{mi % 64 // 16}][{ni % 4}] lane {16 * (ni % 16 // 4) + mi % 16}"
        s += f" got {g!r} want {w!r}"
        if c.fp:
            s += f" digits got {decode(g, nk(c))} want {decode(w, nk(c))}"
        lines.append(s)
    return "\n".join(lines)


# ------------------------------------------------------------------ the library: route and device run
def _fake(i):
    return 4096 * (i + 1)            # a made-up aligned address: the route entry and a refused call dereference nothing


def buffers(c):
    """the pointer fields the case sets"""
    names = ["A", "Bt"] + (["C"] if not c.qkv else ["q", "k", "vt"])
    names += (["bias"] if c.bias else []) + (["addtab"] if c.tab else []) + (["pre_out"] if c.pre_out else []) + (["rowscale"] if c.rowscale else [])
    names += (["aux"] if c.dact != "none" else []) + (["resid"] if c.resid else []) + (["c1", "c0"] if c.op == "colaffine" else [])
    return names


def make_call(c, ptrs=None):
    """the ishara_gemm_nt_call of a case; ptrs: name -> address (default: made-up aligned addresses for everything the case has)"""
    if ptrs is None:
        ptrs = {n: _fake(i) for i, n in enumerate(buffers(c))}
    k = _lib.GemmNtCall()
    for n in buffers(c):
        setattr(k, n, ptrs[n])
    k.dtA, k.dtM, k.dtC, k.op = DT[c.dtA], DT[c.dtM], DT[c.dtC], OP[c.op]
    k.M, k.N, k.K, k.bt_rows, k.ldb = c.M, c.N, c.K, bt_rows(c), ldb(c)
    k.op_seed, k.op_site, k.op_rate = SEED, OP_SITE, (0.5 if c.op == "dropmask" else 0.0)
    k.tab_period, k.act = (c.tab or 1), ACT[c.act]
    k.drop_seed, k.drop_site, k.drop_rate = SEED, EPI_SITE, (0.5 if c.drop else 0.0)
    k.T, k.rowscale_bias, k.dact = (c.T or 1), int(c.rowscale == 2), DACT[c.dact]
    k.mode, k.H, k.dh, k.head_major = (1, *c.qkv) if c.qkv else (0, 1, 1, 1)
    return k


class switches:
    """the debug switch a case runs under, restored on the way out"""
    def __init__(self, lib, c):
        self.lib, self.on = lib, (FORCE[c.route] if c.force else 0)

    def __enter__(self):
        self.lib.ishara_debug_force_regstage(self.on)

    def __exit__(self, *a):
        self.lib.ishara_debug_force_regstage(0)


def route(lib, c):
    """(route, profiler key) of the case from the function the launcher launches from (host only); a refused call: ("NT_REFUSED", "", message)"""
    r, kern = C.c_char_p(), C.c_char_p()
    k = make_call(c)
    with switches(lib, c):
        rc = lib.ishara_debug_gemm_nt_route(C.byref(k), C.byref(r), C.byref(kern))
    assert rc == 0, lib.ishara_last_error()
    return r.value.decode(), kern.value.decode()


def kernel_name(c):
    """the profiler key the row claims"""
    if c.dtM == "f16":
        return "gemm_nt_kernel<f16>"
    if c.route == R_:
        return f"gemm_nt_kernel<{c.dtA},{c.dtM},{c.dtC}>"
    return f"gemm_nt_{'t' if c.route == T_ else 'glds'}_kernel<{c.dtM},{c.dtC}>"


def out_shapes(c):
    s = {}
    if c.qkv:
        B, H, dh, _ = qkv_dims(c)
        s["q"] = s["k"] = (B, H, c.T, dh)
        s["vt"] = (B, H, dh, c.T)
    else:
        s["C"] = (c.M, c.N)
    if c.pre_out:
        s["pre_out"] = (c.M, c.N)
    return s


class Device:
    """the inputs of one case on the device (uploaded once), and fresh guarded outputs per launch"""
    def __init__(self, lib, c, op):
        import torch
        self.lib, self.c, self.torch = lib, c, torch
        self.tdt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
        dev = "cuda"

        def up(x, dt):
            return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(self.tdt[dt]).to(dev)

        Bt = np.zeros((bt_rows(c), ldb(c)))
        Bt[c.N:, :] = np.nan               # read and discarded by every kernel
        Bt[:c.N, :c.K] = op["W"]           # columns [K, ldb) of the real rows stay zero
        self.t = {"A": up(op["A"], c.dtA), "Bt": up(Bt, c.dtM)}
        for n, dt in (("bias", "f32"), ("addtab", "f32"), ("rowscale", "f32"), ("aux", c.dtC), ("resid", c.dtC)):
            if n in op:
                self.t[n] = up(op[n], dt)
        for n in ("c1", "c0"):
            if n in op:
                pad = np.full(-(-c.K // bk(c)) * bk(c), np.nan)
                pad[:c.K] = op[n]
                self.t[n] = up(pad, "f32")

    def masks(self):
        """the dropout masks from ishara_dropout_mask with the call's seed / site / rate"""
        torch, c, m = self.torch, self.c, {}
        for key, on, site, cols in (("op", c.op == "dropmask", OP_SITE, c.K), ("epi", c.drop, EPI_SITE, c.N)):
            if on:
                t = torch.empty(c.M, cols, dtype=torch.float32, device="cuda")
                _lib.check(self.lib.ishara_dropout_mask(SEED, site, c.M, cols, C.c_float(0.5), C.c_void_p(t.data_ptr()), _lib.stream()), "ishara_dropout_mask")
                torch.cuda.synchronize()
                m[key] = t.cpu().numpy().astype(np.float64)
        return m

    def launch(self):
        """one launch into fresh outputs between sentinels; returns name -> fp32 array, plus "guards_ok" """
        torch, c = self.torch, self.c
        es = 4 if c.dtC == "f32" else 2
        g = GUARD * 4 // es                       # guard elements: GUARD floats' worth of bytes on each side
        outs = {}
        for n, shape in out_shapes(c).items():
            k = int(np.prod(shape))
            outs[n] = (torch.full((k + 2 * g,), SENTINEL[c.dtC], dtype=self.tdt[c.dtC], device="cuda"), k)
        ptrs = {n: v.data_ptr() for n, v in self.t.items()}
        ptrs.update({n: v.data_ptr() + g * es for n, (v, _) in outs.items()})
        call = make_call(c, ptrs)
        with switches(self.lib, c):
            rc = self.lib.ishara_op_gemm_nt(C.byref(call), _lib.stream())
            _lib.check(rc, "ishara_op_gemm_nt")
            torch.cuda.synchronize()
        r = {"guards_ok": True}
        for n, (v, k) in outs.items():
            sent = SENTINEL[c.dtC]
            r["guards_ok"] = r["guards_ok"] and bool((v[:g] == sent).all().item()) and bool((v[g + k:] == sent).all().item())
            r[n] = v[g:g + k].float().cpu().numpy().reshape(out_shapes(c)[n])
        return r
