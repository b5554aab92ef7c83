"""CPU: every single-operator entry point refuses what it has no kernel for — unknown dtypes, ISHARA_F16 for the backward operators (fp16
is inference-only) and for every operator of the torch Squeezeformer family, fp16 attention with dropout, classifier routes that do not take
the shape, shapes outside a kernel's range, null or misaligned buffers — with an error and an ishara_last_error()
message of its own, before any HIP call (all device pointers and the stream are NULL here: a call that got as far as a launch would fail
with a HIP error instead, or fault)."""
import ctypes as C

import pytest

from ishara_amd import _lib

F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
BAD_DT = [-1, 3, 7]
N = None


def _ops():
    """name -> callable(dt) with otherwise valid small shapes and NULL pointers"""
    f = C.c_float
    return {
        "ishara_op_dense_fwd": lambda L, dt: L.ishara_op_dense_fwd(dt, N, N, N, N, 64, 256, 64, 0, N, N),
        "ishara_op_dense_fwd_ex": lambda L, dt: L.ishara_op_dense_fwd_ex(dt, N, N, N, N, N, 64, 256, 64, 0, N, N),
        "ishara_op_dense_bwd": lambda L, dt: L.ishara_op_dense_bwd(dt, N, N, N, N, N, N, 64, 256, 64, N, N),
        "ishara_op_layernorm_fwd": lambda L, dt: L.ishara_op_layernorm_fwd(dt, N, N, N, f(1e-6), N, N, N, 64, 256, N),
        "ishara_op_layernorm_bwd": lambda L, dt: L.ishara_op_layernorm_bwd(dt, N, N, N, N, N, N, N, N, 64, 256, N),
        "ishara_op_dwconv_fwd": lambda L, dt: L.ishara_op_dwconv_fwd(dt, 1, N, N, N, N, N, N, 2, 64, 128, 11, 10, N),
        "ishara_op_dwconv_fwd_ex": lambda L, dt: L.ishara_op_dwconv_fwd_ex(dt, 1, N, N, N, N, N, N, N, 2, 64, 128, 11, 10, N),
        "ishara_op_dwconv_bwd": lambda L, dt: L.ishara_op_dwconv_bwd(dt, 1, N, N, N, N, N, N, N, 2, 64, 128, 11, 10, N),
        "ishara_op_bn_bwd_apply": lambda L, dt: L.ishara_op_bn_bwd_apply(dt, N, N, N, N, N, N, N, 0, N, N, 2, 64, 128, N),
        "ishara_op_dwconv_bwd_bn": lambda L, dt: L.ishara_op_dwconv_bwd_bn(dt, 1, N, N, N, N, N, N, N, 0, N, N, N, N, N, N, N, N, 2, 64, 128, 11, 10, N),
        "ishara_op_attn_fwd": lambda L, dt: L.ishara_op_attn_fwd(dt, N, N, 1, 4, 64, 32, f(0.1), 1, 2, f(0.0), 1, N, N),
        "ishara_op_attn_bwd": lambda L, dt: L.ishara_op_attn_bwd(dt, N, N, N, 1, 4, 64, 32, f(0.1), 1, 2, f(0.0), 1, N, N),
        "ishara_op_qkv_fwd": lambda L, dt: L.ishara_op_qkv_fwd(dt, N, N, N, f(1e-6), N, N, N, N, N, 1, 64, 4, 32, 1, N, N),
        "ishara_op_classifier_fwd": lambda L, dt: L.ishara_op_classifier_fwd(dt, N, N, N, N, 64, 256, 60, 0, N, N),
        "ishara_op_gemm_tn": lambda L, dt: _gemm_tn(L, dict(dtA=dt, dtB=dt, dtM=dt)),
        "ishara_op_gemm_nt": lambda L, dt: _gemm_nt(L, dtA=dt, dtM=dt, dtC=dt),
        "ishara_op_gemm_as": lambda L, dt: _gemm_as(L, dtA=dt, dtM=dt, dtC=dt),
        **{n: (lambda L, dt, n=n: _r4_call(L, n, dt=dt)) for n in R4_DEFAULTS},
    }


# ---- the torch Squeezeformer family's operators: name -> (pointer arguments, keyword defaults of the rest, in call order)
R4_DEFAULTS = {
    "ishara_op_relattn_fwd": (9, dict(B=2, H=2, T=33, dh=16, seed=1, site=2, rate=0.0)),
    "ishara_op_relattn_bwd": (14, dict(B=2, H=2, T=33, dh=16, seed=1, site=2, rate=0.0)),
    "ishara_op_r4_subsample_fwd": (6, dict(B=2, T0=30, F=16, d=16)),
    "ishara_op_r4_subsample_bwd": (10, dict(B=2, T0=30, F=16, d=16)),
    "ishara_op_r4_time_reduce_fwd": (7, dict(B=2, Tin=8, d=24)),
    "ishara_op_r4_time_reduce_bwd": (9, dict(B=2, Tin=8, d=24)),
    "ishara_op_r4_rows": (3, dict(B=2, Tdst=8, Tsrc=8, d=16)),
}
R4_OPS = sorted(R4_DEFAULTS)


def _r4_call(L, name, dt=F32, ptrs=None, mode=4, **kw):
    """one call of a torch-Squeezeformer operator: NULL pointers (or `ptrs`), the default shape with `kw` replacing single values; the last
    two arguments (scratch, stream; ishara_op_r4_rows: stream) stay NULL unless `ptrs` is one longer than the pointer count (the scratch)"""
    nptr, defaults = R4_DEFAULTS[name]
    vals = {**defaults, **kw}
    assert set(vals) == set(defaults), (name, kw)
    rest = [C.c_float(v) if k == "rate" else v for k, v in vals.items()]
    ptrs = list(ptrs) if ptrs is not None else [N] * nptr
    if name == "ishara_op_r4_rows":
        return L.ishara_op_r4_rows(dt, mode, *ptrs[:nptr], *rest, N)
    scratch = ptrs[nptr] if len(ptrs) > nptr else N
    return getattr(L, name)(dt, *ptrs[:nptr], *rest, scratch, N)


CTC_LOSS = ["ishara_ctc_loss", "ishara_op_ctc_loss"]
BACKWARD = ["ishara_op_dense_bwd", "ishara_op_layernorm_bwd", "ishara_op_dwconv_bwd", "ishara_op_bn_bwd_apply", "ishara_op_dwconv_bwd_bn", "ishara_op_attn_bwd",
            "ishara_op_gemm_tn"]


def _gemm_tn_call(**kw):
    """one ishara_gemm_tn_call: a plain bf16 call of the transposed-read kernel with made-up aligned addresses, `kw` replacing single fields"""
    k = _lib.GemmTnCall()
    v = dict(A=4096, B=8192, out=12288, dbias=16384, dtA=BF16, dtB=BF16, dtM=BF16, M=576, Ka=128, Nb=128)
    v.update(kw)
    for n, x in v.items():
        setattr(k, n, x)
    return k


PSA_FIELDS = dict(P=20480, Q=24576, W=28672, G=32768, Rpart=36864, psa_T=128, ldw=128, M=1024)


def _gemm_tn(L, *calls, slab=C.c_void_p(1 << 20), d0=N, d1=N):
    """ishara_op_gemm_tn on a list of calls (dicts of field replacements) with a made-up slab and a NULL stream"""
    arr = (_lib.GemmTnCall * len(calls))(*[_gemm_tn_call(**kw) for kw in calls])
    return L.ishara_op_gemm_tn(arr, len(calls), slab, d0, d1, N)


def _gemm_nt_call(**kw):
    """one ishara_gemm_nt_call: a plain bf16 call of the 128 x 128 tile kernel (bias + residual) with made-up aligned addresses, `kw` replacing
    single fields"""
    k = _lib.GemmNtCall()
    v = dict(A=4096, Bt=8192, C=12288, bias=16384, resid=20480, dtA=BF16, dtM=BF16, dtC=BF16, M=200, N=132, K=64, bt_rows=256, ldb=64, tab_period=1,
             T=1, H=1, dh=1, head_major=1)
    v.update(kw)
    for n, x in v.items():
        setattr(k, n, x)
    return k


def _gemm_nt(L, **kw):
    return L.ishara_op_gemm_nt(C.byref(_gemm_nt_call(**kw)), N)


def _gemm_nt_route(L, **kw):
    """(rc, route, kernel) of ishara_debug_gemm_nt_route"""
    route, kernel = C.c_char_p(), C.c_char_p()
    rc = L.ishara_debug_gemm_nt_route(C.byref(_gemm_nt_call(**kw)), C.byref(route), C.byref(kernel))
    return rc, route.value, kernel.value


def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the operator's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


def test_every_dtype_taking_operator_is_listed():
    """every ishara_op_* with a dtype argument (first argument; ishara_op_gemm_tn: the three dtypes of each call of its list) is covered
    below; ishara_op_ctc_loss (fp32 only, no dtype argument) has its refusals with ishara_ctc_loss and ishara_greedy_decode at the end of
    this file"""
    with_dt = {n for n, (_, args) in _lib.SIGNATURES.items() if n.startswith("ishara_op_") and not n.endswith("_bytes")
               and not n.startswith("ishara_op_log_softmax") and n not in CTC_LOSS}
    assert with_dt == set(_ops())
    assert set(CTC_LOSS) <= set(_lib.SIGNATURES)


@pytest.mark.parametrize("dt", BAD_DT)
@pytest.mark.parametrize("name", sorted(_ops()))
def test_unknown_dtype_is_refused(lib, name, dt):
    _refused(lib, _ops()[name](lib, dt), name, "unknown dtype", str(dt))


@pytest.mark.parametrize("name", BACKWARD)
def test_backward_operators_refuse_f16(lib, name):
    _refused(lib, _ops()[name](lib, F16), name, "ISHARA_F16", "inference-only")


@pytest.mark.parametrize("name", R4_OPS)
def test_torch_squeezeformer_operators_refuse_f16(lib, name):
    """the family has no fp16 kernels (its typed launches would read ISHARA_F16 buffers as float): forward and backward alike"""
    _refused(lib, _r4_call(lib, name, dt=F16), name, "ISHARA_F16", "no fp16 kernels")


@pytest.mark.parametrize("name", ["ishara_op_relattn_fwd", "ishara_op_relattn_bwd"])
@pytest.mark.parametrize("kw,word", [(dict(dh=12), "head dim"), (dict(dh=128), "head dim"), (dict(dh=0), "head dim"), (dict(T=0), ">= 1"), (dict(B=0), ">= 1"),
                                     (dict(B=-2), ">= 1"), (dict(H=0), ">= 1"), (dict(rate=1.0), "rate"), (dict(rate=-0.1), "rate"), (dict(rate=float("nan")), "rate"),
                                     (dict(B=40000, H=2), "too large")])
def test_relattn_refuses_shapes_and_rates(lib, name, kw, word):
    _refused(lib, _r4_call(lib, name, **kw), name, word)
    assert lib.ishara_op_relattn_scratch_bytes(2, 2, 33, 12) < 0 and lib.ishara_op_relattn_scratch_bytes(2, 2, 0, 16) < 0
    assert lib.ishara_op_relattn_scratch_bytes(2, 2, 33, 16) > 0


@pytest.mark.parametrize("name", ["ishara_op_r4_subsample_fwd", "ishara_op_r4_subsample_bwd"])
@pytest.mark.parametrize("kw,word", [(dict(T0=6), ">= 7"), (dict(F=6), ">= 7"), (dict(T0=0), ">= 7"), (dict(B=0), ">= 1"), (dict(d=0), ">= 1")])
def test_subsample_refuses_shapes(lib, name, kw, word):
    _refused(lib, _r4_call(lib, name, **kw), name, word)
    assert lib.ishara_op_r4_subsample_scratch_bytes(2, 6, 16, 16) < 0 and lib.ishara_op_r4_subsample_scratch_bytes(2, 7, 7, 16) > 0


@pytest.mark.parametrize("name", ["ishara_op_r4_time_reduce_fwd", "ishara_op_r4_time_reduce_bwd"])
@pytest.mark.parametrize("kw,word", [(dict(Tin=2), ">= 3"), (dict(d=2), ">= 3"), (dict(d=20), "multiple of 8"), (dict(B=0), ">= 1")])
def test_time_reduce_refuses_shapes(lib, name, kw, word):
    _refused(lib, _r4_call(lib, name, **kw), name, word)
    assert lib.ishara_op_r4_time_reduce_scratch_bytes(2, 2, 24) < 0 and lib.ishara_op_r4_time_reduce_scratch_bytes(2, 3, 24) > 0


@pytest.mark.parametrize("mode", [-1, 5, 100])
def test_rows_refuses_unknown_modes(lib, mode):
    _refused(lib, _r4_call(lib, "ishara_op_r4_rows", mode=mode), "ishara_op_r4_rows", "unknown mode", str(mode))


@pytest.mark.parametrize("mode,kw,word", [(0, dict(Tdst=17, Tsrc=8), "past the source"), (1, dict(Tdst=9, Tsrc=8), "past the source"), (2, dict(Tdst=5, Tsrc=8), "past the source"),
                                          (4, dict(Tdst=8, Tsrc=9), "past the source"), (3, dict(B=0), "bad shape"), (3, dict(d=0), "bad shape"), (3, dict(Tdst=0), "bad shape")])
def test_rows_refuses_shapes(lib, mode, kw, word):
    _refused(lib, _r4_call(lib, "ishara_op_r4_rows", mode=mode, **kw), "ishara_op_r4_rows", word)


@pytest.mark.parametrize("name", R4_OPS)
def test_torch_squeezeformer_operators_refuse_null_and_misaligned_buffers(lib, name):
    """valid shapes with every pointer NULL, with one required pointer NULL, and with one pointer off a 16-byte boundary (the other addresses
    are made up: a refused call dereferences nothing)"""
    nptr = R4_DEFAULTS[name][0]
    _refused(lib, _r4_call(lib, name), name, "null")
    good = [C.c_void_p(4096 * (i + 1)) for i in range(nptr + 1)]
    _refused(lib, _r4_call(lib, name, ptrs=good[:0] + [N] + good[1:]), name, "null")
    for i in (0, nptr - 1, nptr):
        if name == "ishara_op_r4_rows" and i == nptr:
            continue
        bad = list(good)
        bad[i] = C.c_void_p(4096 * (i + 1) + 8)
        _refused(lib, _r4_call(lib, name, ptrs=bad), name, "misaligned")


def test_f16_attention_refuses_dropout(lib):
    rc = lib.ishara_op_attn_fwd(F16, N, N, 1, 4, 64, 32, C.c_float(0.1), 1, 2, C.c_float(0.1), 1, N, N)
    _refused(lib, rc, "ishara_op_attn_fwd", "dropout")


# ---- ishara_op_attn_fwd / _bwd: shapes, rates, impl values and buffers are refused before the first launch (the qkv split of the forward)
ATTN_OPS = {"ishara_op_attn_fwd": 2, "ishara_op_attn_bwd": 3}      # name -> operand pointers (qkv, o / o, dout, dqkv)
ATTN_OPERANDS = {"ishara_op_attn_fwd": ("qkv", "o"), "ishara_op_attn_bwd": ("o", "dout", "dqkv")}


def _attn_call(L, name, dt=BF16, ptrs=None, scratch=C.c_void_p(1 << 20), **kw):
    """one call with made-up aligned addresses (a refused call dereferences nothing) or `ptrs`; `kw` replaces single values of the default shape"""
    v = dict(B=1, H=4, T=64, dh=32, rate=0.0, impl=1)
    assert set(kw) <= set(v), kw
    v.update(kw)
    n = ATTN_OPS[name]
    ptrs = list(ptrs) if ptrs is not None else [C.c_void_p(4096 * (i + 1)) for i in range(n)]
    return getattr(L, name)(dt, *ptrs, v["B"], v["H"], v["T"], v["dh"], C.c_float(0.1), 1, 2, C.c_float(v["rate"]), v["impl"], scratch, N)


ATTN_REFUSALS = [(dict(B=0), ">= 1"), (dict(B=-1), ">= 1"), (dict(H=0), ">= 1"), (dict(T=0), ">= 1"), (dict(T=-8), ">= 1"),
                 (dict(dh=0), "head dim 0"), (dict(dh=12), "head dim 12"), (dict(dh=40), "head dim 40"), (dict(dh=128), "head dim 128"),
                 (dict(T=60), "T % 8"), (dict(T=1, dh=64), "T % 8"), (dict(T=60, impl=2), "T % 8"),
                 (dict(rate=1.0), "rate"), (dict(rate=-0.1), "rate"), (dict(rate=float("nan")), "rate"),
                 (dict(impl=-1), "unknown impl"), (dict(impl=3), "unknown impl"), (dict(impl=2, dh=16), "impl 2"),
                 (dict(B=40000, H=2), "too large"), (dict(B=64, H=64, T=4096, dh=64), "too large")]


@pytest.mark.parametrize("name", sorted(ATTN_OPS))
@pytest.mark.parametrize("kw,word", ATTN_REFUSALS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_attention_refuses_shapes_rates_and_impls(lib, name, kw, word):
    _refused(lib, _attn_call(lib, name, **kw), name, word)


@pytest.mark.parametrize("name", sorted(ATTN_OPS))
def test_attention_takes_any_frame_count_on_the_lane_split_route(lib, name):
    """T % 8 != 0 is refused only where the MFMA kernels would take the call: impl 0, f32 and the head dims without an MFMA kernel pass the shape
    checks (and are refused for the null scratch instead); impl 2 has no lane-split kernels to fall back to"""
    for kw, dt in ((dict(T=61, impl=0), BF16), (dict(T=61, impl=1), F32), (dict(T=61, dh=24), BF16), (dict(T=1, dh=48), BF16)):
        _refused(lib, _attn_call(lib, name, dt=dt, scratch=N, **kw), name, "null scratch")
    _refused(lib, _attn_call(lib, name, dt=F32, impl=2), name, "impl 2")


@pytest.mark.parametrize("name", sorted(ATTN_OPS))
def test_attention_refuses_null_and_misaligned_buffers(lib, name):
    n = ATTN_OPS[name]
    good = [C.c_void_p(4096 * (i + 1)) for i in range(n)]
    who = ATTN_OPERANDS[name]
    _refused(lib, _attn_call(lib, name, ptrs=[N] * n, scratch=N), name, "null " + who[0])
    for i in range(n):      # the message names the operand that is at fault
        _refused(lib, _attn_call(lib, name, ptrs=good[:i] + [N] + good[i + 1:]), name, "null " + who[i])
        for off in (2, 4, 8):
            _refused(lib, _attn_call(lib, name, ptrs=good[:i] + [C.c_void_p(4096 * (i + 1) + off)] + good[i + 1:]), name, "misaligned " + who[i] + ":", "16-byte")
    _refused(lib, _attn_call(lib, name, scratch=N), name, "null scratch")
    for off in (16, 64, 128):
        _refused(lib, _attn_call(lib, name, scratch=C.c_void_p((1 << 20) + off)), name, "misaligned scratch", "256-byte")


def test_attention_scratch_layout_is_consistent_and_refuses_bad_shapes(lib):
    """lse | delta | keep-bit words follow the three operand copies, each region on a 256-byte boundary and inside the scratch"""
    for B, H, T, dh in ((1, 3, 8, 32), (2, 3, 33, 24), (2, 8, 392, 32), (1, 1, 1, 8)):
        out = (C.c_int64 * 6)()
        assert lib.ishara_op_attn_scratch_layout_bytes(B, H, T, dh, out) == 0
        total = lib.ishara_op_attn_scratch_bytes(B, H, T, dh)
        (lo, le), (do, de), (mo, me) = ((out[2 * i], out[2 * i + 1]) for i in range(3))
        assert le == de == 4 * B * H * T and me == 4 * 256 * B * H * ((T + 127) // 128) * ((T + 63) // 64)
        assert lo >= 3 * 4 * B * H * T * dh and lo + le <= do and do + de <= mo and mo + me <= total
        assert lo % 256 == do % 256 == mo % 256 == total % 256 == 0 and total - (mo + me) < 256 and do - (lo + le) < 256 and mo - (do + de) < 256
    _refused(lib, lib.ishara_op_attn_scratch_layout_bytes(1, 3, 0, 32, (C.c_int64 * 6)()), "ishara_op_attn_scratch_layout_bytes", ">= 1")
    _refused(lib, lib.ishara_op_attn_scratch_layout_bytes(1, 3, 8, 32, None), "ishara_op_attn_scratch_layout_bytes", "null")


# ---- the depthwise-conv backward operators: ishara_op_dwconv_bwd, ishara_op_dwconv_bwd_bn and ishara_op_bn_bwd_apply refuse shapes, a padl
# outside the kernel and null or misaligned operands before any HIP call
DWB_OPERANDS = {      # name -> (required operands in call order, optional ones)
    "ishara_op_dwconv_bwd": (("dy", "x", "w", "dx", "dw"), ("dbias", "scratch")),
    "ishara_op_bn_bwd_apply": (("dy", "h", "mean", "rstd", "a", "E", "Fc", "dx"), ("sg",)),
    "ishara_op_dwconv_bwd_bn": (("dy", "h", "mean", "rstd", "a", "E", "Fc", "x", "w", "dx", "dw", "tmp"), ("sg", "dbias", "scratch")),
}


def _dwb_call(L, name, dt=BF16, ptrs=None, **kw):
    """one call with made-up aligned addresses (a refused call dereferences nothing); `ptrs` replaces single operands by name, `kw` single
    values of the default shape"""
    v = dict(B=2, T=64, C=128, k=11, padl=10)
    assert set(kw) <= set(v), kw
    v.update(kw)
    req, opt = DWB_OPERANDS[name]
    p = {n: C.c_void_p(4096 * (i + 1)) for i, n in enumerate(req + opt)}
    p.update(ptrs or {})
    if name == "ishara_op_bn_bwd_apply":
        return L.ishara_op_bn_bwd_apply(dt, p["dy"], p["h"], p["mean"], p["rstd"], p["a"], p["sg"], p["E"], 0, p["Fc"], p["dx"], v["B"], v["T"], v["C"], N)
    shape = (v["B"], v["T"], v["C"], v["k"], v["padl"], N)
    if name == "ishara_op_dwconv_bwd":
        return L.ishara_op_dwconv_bwd(dt, 1, p["dy"], p["x"], p["w"], p["dx"], p["dw"], p["dbias"], p["scratch"], *shape)
    return L.ishara_op_dwconv_bwd_bn(dt, 1, p["dy"], p["h"], p["mean"], p["rstd"], p["a"], p["sg"], p["E"], 0, p["Fc"], p["x"], p["w"], p["dx"], p["dw"], p["dbias"],
                                     p["scratch"], p["tmp"], *shape)


DWB_SHAPES = [(dict(B=0), ">= 1"), (dict(B=-3), ">= 1"), (dict(T=0), ">= 1"), (dict(T=-1), ">= 1"), (dict(B=65536), "too large"),
              (dict(C=0), "multiple of 8"), (dict(C=12), "multiple of 8"), (dict(C=-8), "multiple of 8")]
DWB_KERNELS = [(dict(k=0, padl=0), "kernel size 0"), (dict(k=32, padl=0), "kernel size 32"), (dict(k=-1, padl=0), "kernel size -1"),
               (dict(padl=-1), "padl=-1"), (dict(padl=11), "padl=11"), (dict(k=1, padl=1), "padl=1"), (dict(k=5, padl=5), "padl=5")]


DWB_ROWS = [(n, kw, word) for n in sorted(DWB_OPERANDS) for kw, word in DWB_SHAPES + (DWB_KERNELS if n != "ishara_op_bn_bwd_apply" else [])]      # (the BatchNorm backward has no kernel size)


@pytest.mark.parametrize("name,kw,word", DWB_ROWS, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_dwconv_backward_refuses_shapes_and_paddings(lib, name, kw, word):
    _refused(lib, _dwb_call(lib, name, **kw), name, word)


@pytest.mark.parametrize("name", sorted(DWB_OPERANDS))
def test_dwconv_backward_refuses_null_and_misaligned_buffers(lib, name):
    req, opt = DWB_OPERANDS[name]
    for i, n in enumerate(req):      # the message names the operand at fault
        _refused(lib, _dwb_call(lib, name, ptrs={n: N}), name, "null " + n)
        for off in (2, 4, 8):
            _refused(lib, _dwb_call(lib, name, ptrs={n: C.c_void_p(4096 * (i + 1) + off)}), name, "misaligned " + n + ":", "16-byte")
    for n in opt:                    # optional operands may be NULL (the call then gets as far as the next check) but not off 16 bytes
        _refused(lib, _dwb_call(lib, name, ptrs={n: C.c_void_p(1 << 20 | 8)}), name, "misaligned optional", "16-byte")
        _refused(lib, _dwb_call(lib, name, ptrs={n: N, req[0]: N}), name, "null " + req[0])
    for dt in (F32, BF16):           # the checks do not depend on the dtype
        _refused(lib, _dwb_call(lib, name, dt=dt, ptrs={req[-1]: N}), name, "null " + req[-1])


# (dt, M, K, C, route): shapes / dtypes the named route has no kernel for
@pytest.mark.parametrize("dt,M,K,C_,route,why", [
    (F32, 64, 256, 60, 1, "16-bit"),            # A-stationary: 16-bit operands only
    (F32, 64, 256, 60, 2, "16-bit"),            # dense_narrow: 16-bit operands only
    (F16, 64, 256, 62, 1, "C % 4"),             # A-stationary: whole 16-byte groups of the 64-column tile
    (BF16, 64, 256, 68, 1, "C <= 64"),
    (F16, 64, 128, 60, 1, "K 256 / 512"),
    (BF16, 64, 1024, 60, 1, "K 256 / 512"),
    (F16, 64, 256, 65, 2, "C <= 64"),           # dense_narrow: one lane per class
    (BF16, 64, 48, 60, 2, "K % 32"),
    (F16, 64, 100, 60, 3, "16-byte"),           # GEMM: 16-byte operand rows
    (F32, 64, 250, 60, 3, "16-byte"),
])
def test_classifier_refuses_routes_the_shape_cannot_take(lib, dt, M, K, C_, route, why):
    rc = lib.ishara_op_classifier_fwd(dt, N, N, N, N, M, K, C_, route, N, N)
    _refused(lib, rc, "ishara_op_classifier_fwd", f"route {route}", why)


@pytest.mark.parametrize("route", [-1, 4])
def test_classifier_refuses_unknown_routes(lib, route):
    _refused(lib, lib.ishara_op_classifier_fwd(F16, N, N, N, N, 64, 256, 60, route, N, N), "ishara_op_classifier_fwd", "unknown route")


def test_classifier_auto_route_of_an_untakeable_shape_is_refused(lib):
    """route 0 on a 16-bit K that no route takes (K % 8 != 0) resolves to the GEMM, which refuses it"""
    _refused(lib, lib.ishara_op_classifier_fwd(F16, N, N, N, N, 64, 100, 60, 0, N, N), "ishara_op_classifier_fwd", "route 3")


@pytest.mark.parametrize("B,T,H,dh,head_major", [(1, 60, 4, 32, 1), (1, 64, 4, 12, 1), (1, 64, 4, 32, 2), (0, 64, 4, 32, 1)])
def test_qkv_refuses_shapes_without_a_kernel(lib, B, T, H, dh, head_major):
    rc = lib.ishara_op_qkv_fwd(F16, N, N, N, C.c_float(1e-6), N, N, N, N, N, B, T, H, dh, head_major, N, N)
    _refused(lib, rc, "ishara_op_qkv_fwd", "unsupported")


def test_qkv_refuses_null_buffers_before_launching(lib):
    rc = lib.ishara_op_qkv_fwd(F16, N, N, N, C.c_float(1e-6), N, N, N, N, N, 1, 64, 4, 32, 1, N, N)
    _refused(lib, rc, "ishara_op_qkv_fwd", "null")
    assert lib.ishara_op_qkv_scratch_bytes(1, 64, 4, 32) > 0 and lib.ishara_op_qkv_scratch_bytes(0, 64, 4, 32) < 0


# ---- the module probe (ishara_debug_module_*): refusals that need no device
def _handle(**kw):
    from ishara_amd import make_config
    from ishara_amd.model import Model
    return Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, max_batch=4, **kw), device=None)


def _probe_calls(lib, h, i, B, training=0):
    f = C.c_float
    return {
        "ishara_debug_module_forward": lambda: lib.ishara_debug_module_forward(h, i, N, B, N, training, 1, N),
        "ishara_debug_module_backward": lambda: lib.ishara_debug_module_backward(h, i, N, B, N, N),
        "ishara_debug_head_loss_backward": lambda: lib.ishara_debug_head_loss_backward(h, N, N, B, N, N, f(1.0), N, N),
    }


@pytest.mark.parametrize("name", ["ishara_debug_module_forward", "ishara_debug_module_backward", "ishara_debug_head_loss_backward"])
def test_probe_refuses_an_unbound_handle(lib, name):
    m = _handle()
    _refused(lib, _probe_calls(lib, m._h, 1, 2)[name](), name, "not bound")


@pytest.mark.parametrize("name", ["ishara_debug_module_forward", "ishara_debug_module_backward"])
@pytest.mark.parametrize("i", [-1, 16, 100])
def test_probe_refuses_a_module_index_out_of_range(lib, name, i):
    m = _handle()
    assert lib.ishara_debug_module_count(m._h) == 16      # stem, 2 x (3 Conv1DBlocks, 4 sub-modules), head
    _refused(lib, _probe_calls(lib, m._h, i, 2)[name](), name, "module index", str(i))


@pytest.mark.parametrize("name", ["ishara_debug_module_forward", "ishara_debug_module_backward", "ishara_debug_head_loss_backward"])
@pytest.mark.parametrize("B", [0, -3, 5])
def test_probe_refuses_a_batch_outside_the_plan(lib, name, B):
    m = _handle()
    _refused(lib, _probe_calls(lib, m._h, 1, B)[name](), name, "batch", "1..4")


def test_probe_refuses_fp16_training_and_lists_fp16_modules(lib):
    m = _handle(dtype="f16")
    _refused(lib, _probe_calls(lib, m._h, 1, 2, training=1)["ishara_debug_module_forward"](), "ishara_debug_module_forward", "ISHARA_F16", "training=1")
    _refused(lib, _probe_calls(lib, m._h, 1, 2)["ishara_debug_module_backward"](), "ishara_debug_module_backward", "ISHARA_F16")
    _refused(lib, _probe_calls(lib, m._h, 1, 2, training=0)["ishara_debug_module_forward"](), "ishara_debug_module_forward", "not bound")      # inference is not refused for the dtype


def test_probe_refuses_the_encoder_families(lib):
    from ishara_amd import make_config
    cfg = make_config(dim=64, num_conv_squeeze_blocks=0, num_conv_conform_blocks=1, num_heads=4, input_shape=(64, 64), max_batch=2, dtype="f32")
    cfg.family = _lib.FAMILY_TORCH_CONFORMER
    h = C.c_void_p()
    assert lib.ishara_create(C.byref(cfg), C.byref(h)) == 0, lib.ishara_last_error()
    try:
        assert lib.ishara_debug_module_count(h) < 0
        _refused(lib, -1, "ishara_debug_module_count", "ISHARA_FAMILY_KERAS_HYBRID")
        for name, call in _probe_calls(lib, h, 0, 1).items():
            _refused(lib, call(), name, "ISHARA_FAMILY_KERAS_HYBRID")
        _refused(lib, lib.ishara_debug_module_info(h, 0, N, N, N, N, N), "ishara_debug_module_info", "ISHARA_FAMILY_KERAS_HYBRID")
    finally:
        lib.ishara_destroy(h)


# ---- CTC loss (both entry points) and greedy decode: refused before any HIP call, each with its own message
def _ctc_call(lib_, name, ptrs=None, dlb=N, **kw):
    """one call with made-up non-null addresses (a refused call dereferences nothing) or `ptrs` = dict of logits, labels, nll, dlogits, ws"""
    v = dict(B=2, T=16, C=60, L=8, blank=59)
    assert set(kw) <= set(v), kw
    v.update(kw)
    p = dict(logits=C.c_void_p(4096), labels=C.c_void_p(8192), nll=C.c_void_p(12288), dlogits=C.c_void_p(16384), ws=C.c_void_p(20480))
    p.update(ptrs or {})
    tail = (dlb, N) if name == "ishara_op_ctc_loss" else (N,)
    return getattr(lib_, name)(p["logits"], p["labels"], v["B"], v["T"], v["C"], v["L"], v["blank"], p["nll"], p["dlogits"], C.c_float(1.0), p["ws"], *tail)


def _decode_call(lib_, ptrs=None, **kw):
    v = dict(B=2, T=16, C=60, blank=59)
    assert set(kw) <= set(v), kw
    v.update(kw)
    p = dict(logits=C.c_void_p(4096), out_idx=C.c_void_p(8192), out_len=C.c_void_p(12288))
    p.update(ptrs or {})
    return lib_.ishara_greedy_decode(p["logits"], v["B"], v["T"], v["C"], v["blank"], p["out_idx"], p["out_len"], N)


CTC_SHAPES = [(dict(B=-1), ("B=-1",)), (dict(T=0), ("T=0",)), (dict(T=-5), ("T=-5",)), (dict(L=0), ("L=0", "1..255")), (dict(L=256), ("L=256", "1..255")),
              (dict(C=1, blank=0), ("C=1", "2..64")), (dict(C=65, blank=64), ("C=65", "2..64")), (dict(blank=-1), ("blank -1", "0..59")),
              (dict(blank=60), ("blank 60", "0..59")), (dict(C=5, blank=5), ("blank 5", "0..4"))]


@pytest.mark.parametrize("name", CTC_LOSS)
@pytest.mark.parametrize("kw,words", CTC_SHAPES, ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_ctc_loss_refuses_shapes(lib, name, kw, words):
    _refused(lib, _ctc_call(lib, name, **kw), name, *words)


@pytest.mark.parametrize("name", CTC_LOSS)
def test_ctc_loss_refuses_a_frame_count_its_lds_request_cannot_hold(lib, name):
    """one workgroup asks for 4 T + 256 ceil((2L+1)/64) bytes of dynamic LDS next to 4112 static ones (the class rows of the gradient phase,
    log p, the label count and flag) and is launched within the 64 KiB every launch is granted: 4 T + 256 NS <= 61424"""
    for L_, ns in ((8, 1), (255, 8)):
        tmax = (65536 - 4112 - 256 * ns) // 4
        _refused(lib, _ctc_call(lib, name, T=tmax + 1, L=L_), name, f"T={tmax + 1}", "LDS", "61424", f"T <= {tmax}")
        _refused(lib, _ctc_call(lib, name, T=tmax, L=L_, ptrs=dict(ws=N)), name, "null")      # T = tmax passes the shape checks
    _refused(lib, _ctc_call(lib, name, T=2 ** 31 - 1), name, "LDS")


@pytest.mark.parametrize("name", CTC_LOSS)
def test_ctc_loss_refuses_null_and_misaligned_buffers(lib, name):
    for k in ("logits", "labels", "nll", "ws"):
        _refused(lib, _ctc_call(lib, name, ptrs={k: N}), name, "null")
    for off in (1, 2, 4):
        _refused(lib, _ctc_call(lib, name, ptrs=dict(ws=C.c_void_p(20480 + off))), name, "ws", "8-byte")
    if name == "ishara_op_ctc_loss":
        for off in (1, 2, 3):
            _refused(lib, _ctc_call(lib, name, dlb=C.c_void_p(24576 + off)), name, "dlb", "4-byte")


@pytest.mark.parametrize("name", CTC_LOSS)
def test_ctc_loss_of_an_empty_batch_is_a_no_op(lib, name):
    """B == 0 returns 0 without a launch, whatever the pointers; the shape checks still hold"""
    assert _ctc_call(lib, name, B=0, ptrs=dict(logits=N, labels=N, nll=N, dlogits=N, ws=N)) == 0
    _refused(lib, _ctc_call(lib, name, B=0, L=300), name, "L=300")


@pytest.mark.parametrize("kw,words", [(dict(B=-1), ("B=-1",)), (dict(T=0), ("T=0",)), (dict(T=4097), ("T=4097", "4096")), (dict(C=0, blank=0), ("C=0",)),
                                      (dict(blank=-1), ("blank -1", "0..59")), (dict(blank=60), ("blank 60", "0..59")), (dict(C=100, blank=100), ("blank 100", "0..99"))],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_greedy_decode_refuses_shapes(lib, kw, words):
    _refused(lib, _decode_call(lib, **kw), "ishara_greedy_decode", *words)


def test_greedy_decode_refuses_null_buffers_and_skips_an_empty_batch(lib):
    for k in ("logits", "out_idx", "out_len"):
        _refused(lib, _decode_call(lib, ptrs={k: N}), "ishara_greedy_decode", "null")
    assert _decode_call(lib, B=0, ptrs=dict(logits=N, out_idx=N, out_len=N)) == 0


# ---- ishara_op_gemm_tn: the list, the slabs and every call are checked before the first launch; what launch_gemm_tn itself refuses comes back
# with the launcher's message behind the entry's name and the call's index
GEMM_TN_REFUSALS = [
    (dict(A=0), ("null A / B / out",)), (dict(B=0), ("null A / B / out",)), (dict(out=0), ("null A / B / out",)),
    (dict(out=12290), ("misaligned",)), (dict(dbias=16386), ("misaligned",)), (dict(bias_rowscale=40962, bias_T=32), ("misaligned",)),
    (dict(A=4104), ("gemm_tn: operand rows must be 16-byte aligned",)), (dict(B=8200), ("gemm_tn: operand rows must be 16-byte aligned",)),
    (dict(Ka=12, M=100), ("gemm_tn: operand rows must be 16-byte aligned",)),
    (dict(M=0), ("gemm_tn: bad shape",)), (dict(Ka=-128), ("gemm_tn: bad shape",)), (dict(Nb=0), ("gemm_tn: bad shape",)),
    (dict(dtA=F16), ("ISHARA_F16", "dtA")), (dict(dtM=F16), ("ISHARA_F16", "dtM")), (dict(dtB=5), ("unknown dtype", "dtB=5")),
    (dict(dtA=F32, dtB=F32), ("gemm_tn: unsupported dtype combination",)), (dict(dtM=F32), ("gemm_tn: unsupported dtype combination",)),
    (dict(bias_rowscale=40960, bias_T=48), ("gemm_tn: bias row scale needs",)), (dict(bias_rowscale=40960, bias_T=0), ("gemm_tn: bias row scale needs",)),
    (dict(bias_rowscale=40960, bias_T=32, M=130), ("gemm_tn: bias row scale needs",)),
    (dict(ka_valid=100, dbias=0, M=130), ("gemm_tn: padded A columns need",)), (dict(nb_valid=60, Ka=136), ("gemm_tn: padded A columns need",)),
    (dict(ka_valid=100), ("gemm_tn: padded A columns with a bias gradient",)), (dict(nb_valid=62), ("gemm_tn: nb_valid 62 must be a multiple of 4",)),
    (dict(PSA_FIELDS, M=11 * 128), ("gemm_tn: per-sample affine needs",)), (dict(PSA_FIELDS, psa_T=96, M=768), ("gemm_tn: per-sample affine needs",)),
    (dict(PSA_FIELDS, G=0), ("gemm_tn: per-sample affine needs",)), (dict(PSA_FIELDS, psa_T=0), ("gemm_tn: per-sample affine needs",)),
    (dict(PSA_FIELDS, ka_valid=100, dbias=0), ("gemm_tn: per-sample affine needs",)), (dict(PSA_FIELDS, M=1000), ("gemm_tn: per-sample affine needs",)),
    (dict(PSA_FIELDS, bias_rowscale=40960, bias_T=64), ("gemm_tn: per-sample affine needs",)),
    (dict(PSA_FIELDS, ldw=120), ("ldw=120",)), (dict(PSA_FIELDS, W=28673), ("misaligned",)), (dict(PSA_FIELDS, Rpart=36866), ("misaligned",)),
]


@pytest.mark.parametrize("kw,words", GEMM_TN_REFUSALS)
def test_gemm_tn_refuses_buffers_dtypes_and_shapes(lib, kw, words):
    _refused(lib, _gemm_tn(lib, kw), "ishara_op_gemm_tn", "call 0", *words)
    # the same call behind a good one: nothing of the list is launched, and the message names the call
    _refused(lib, _gemm_tn(lib, {}, kw), "ishara_op_gemm_tn", "call 1", *words)
    _refused(lib, _gemm_tn(lib, kw, d0=C.c_void_p(2 << 20), d1=C.c_void_p(3 << 20)), "ishara_op_gemm_tn", "call 0", *words)


def test_gemm_tn_refuses_a_bad_list_or_slab(lib):
    name = "ishara_op_gemm_tn"
    arr = (_lib.GemmTnCall * 1)(_gemm_tn_call())
    _refused(lib, lib.ishara_op_gemm_tn(None, 1, C.c_void_p(1 << 20), N, N, N), name, "null or empty call list")
    _refused(lib, lib.ishara_op_gemm_tn(arr, 0, C.c_void_p(1 << 20), N, N, N), name, "null or empty call list")
    _refused(lib, _gemm_tn(lib, {}, slab=N), name, "slab")
    _refused(lib, _gemm_tn(lib, {}, slab=C.c_void_p((1 << 20) + 8)), name, "misaligned slab")
    _refused(lib, _gemm_tn(lib, {}, d0=C.c_void_p(2 << 20)), name, "both defer_slab0 and defer_slab1")
    _refused(lib, _gemm_tn(lib, {}, d1=C.c_void_p(2 << 20)), name, "both defer_slab0 and defer_slab1")
    _refused(lib, _gemm_tn(lib, {}, d0=C.c_void_p((2 << 20) + 4), d1=C.c_void_p(3 << 20)), name, "misaligned defer slab")
    _refused(lib, _gemm_tn(lib, {}, d0=C.c_void_p(2 << 20), d1=C.c_void_p(2 << 20)), name, "three buffers")
    _refused(lib, _gemm_tn(lib, {}, d0=C.c_void_p(1 << 20), d1=C.c_void_p(2 << 20)), name, "three buffers")


def test_gemm_tn_scratch_query_and_plan_entry_refuse_bad_arguments(lib):
    good = (_lib.GemmTnCall * 2)(_gemm_tn_call(), _gemm_tn_call(M=4096, Ka=512, Nb=768))
    assert lib.ishara_op_gemm_tn_scratch_bytes(good, 2) == 512 * (512 * 768 + 768) * 4          # the larger call's slab: 512 splits' worth
    assert lib.ishara_op_gemm_tn_scratch_bytes(good, 1) == 512 * (128 * 128 + 128) * 4
    assert lib.ishara_op_gemm_tn_scratch_bytes(None, 1) == -1 and lib.ishara_op_gemm_tn_scratch_bytes(good, 0) == -1
    for kw in (dict(M=0), dict(Ka=0), dict(Nb=-1), dict(dtM=F16), dict(dtM=9)):
        assert lib.ishara_op_gemm_tn_scratch_bytes((_lib.GemmTnCall * 1)(_gemm_tn_call(**kw)), 1) == -1, kw
    route, kernel, splits, rps = C.c_char_p(), C.c_char_p(), C.c_int32(), C.c_int32()
    k = _gemm_tn_call()
    _refused(lib, lib.ishara_debug_gemm_tn_plan(None, C.byref(route), C.byref(kernel), C.byref(splits), C.byref(rps)), "ishara_debug_gemm_tn_plan", "null")
    _refused(lib, lib.ishara_debug_gemm_tn_plan(C.byref(k), None, C.byref(kernel), C.byref(splits), C.byref(rps)), "ishara_debug_gemm_tn_plan", "null")
    assert lib.ishara_debug_gemm_tn_plan(C.byref(k), C.byref(route), C.byref(kernel), C.byref(splits), C.byref(rps)) == 0
    assert (route.value, kernel.value, splits.value, rps.value) == (b"TN_TR", b"gemm_tn_tr_kernel<0>", 2, 288)
    k = _gemm_tn_call(dtA=F16)
    assert lib.ishara_debug_gemm_tn_plan(C.byref(k), C.byref(route), C.byref(kernel), C.byref(splits), C.byref(rps)) == 0
    assert (route.value, kernel.value, splits.value, rps.value) == (b"TN_REFUSED", b"", 0, 0) and b"ISHARA_F16" in lib.ishara_last_error()


# ---- ishara_op_gemm_nt / ishara_debug_gemm_nt_route: everything a launch would fault on is refused before any HIP call with a message that names
# the field; what launch_gemm_nt itself refuses comes back with the launcher's message behind the entry's name.  The route entry answers
# "NT_REFUSED" with the same message
QKV_FIELDS = dict(mode=1, q=24576, k=28672, vt=32768, C=0, resid=0, T=40, H=2, dh=32, M=160, N=192, bt_rows=256)
GEMM_NT_REFUSALS = [
    (dict(dtA=5), ("unknown dtype", "dtA=5")), (dict(dtM=-1), ("unknown dtype", "dtM=-1")), (dict(dtC=3), ("unknown dtype", "dtC=3")),
    (dict(op=5), ("unknown op=5",)), (dict(op=-1), ("unknown op=-1",)), (dict(op=3), ("OP_ROWSCALE",)), (dict(op=2), ("OP_COLAFFINE", "c1 / c0")),
    (dict(act=3), ("unknown act=3",)), (dict(dact=3), ("unknown dact=3",)), (dict(mode=2), ("unknown mode=2",)), (dict(head_major=2), ("head_major=2",)),
    (dict(rowscale_bias=2), ("rowscale_bias=2",)), (dict(drop_rate=1.0), ("drop_rate",)), (dict(op_rate=-0.5), ("op_rate",)), (dict(drop_rate=float("nan")), ("drop_rate",)),
    (dict(A=0), ("null A",)), (dict(Bt=0), ("null Bt",)), (dict(C=0), ("null C",)),
    (dict(A=4104), ("gemm_nt: A rows must be 16-byte aligned",)), (dict(Bt=8200), ("misaligned Bt", "16-byte")),
    (dict(C=12292), ("misaligned C", "8-byte")), (dict(C=12296, dtC=F32), ("misaligned C", "16-byte")), (dict(resid=20484), ("misaligned resid",)),
    (dict(pre_out=40964), ("misaligned pre_out",)), (dict(dact=2, aux=40962), ("misaligned aux",)), (dict(bias=16386), ("misaligned bias", "4-byte")),
    (dict(addtab=40968), ("misaligned addtab", "16-byte")), (dict(rowscale=40961, T=8), ("misaligned rowscale",)),
    (dict(op=2, c1=40960, c0=45058, K=72, ldb=128), ("misaligned c0",)),
    (dict(bt_rows=255), ("bt_rows=255", "roundup(N=132, 128)")), (dict(bt_rows=128), ("bt_rows=128",)), (dict(bt_rows=0), ("bt_rows=0",)),
    (dict(K=72, ldb=72), ("ldb=72", "roundup(K=72, 64)")), (dict(K=72, ldb=64), ("ldb=64",)), (dict(dtA=F32, dtM=F32, dtC=F32, K=36, ldb=36), ("ldb=36", "roundup(K=36, 32)")),
    (dict(K=128, ldb=64), ("ldb=64", "roundup(K=128, 32)")), (dict(K=72, ldb=132), ("ldb=132", "16-byte")),
    (dict(addtab=40960, tab_period=0), ("addtab", "tab_period=0")), (dict(addtab=40960, tab_period=-3), ("tab_period=-3",)),
    (dict(rowscale=40960, T=0), ("rowscale", "T=0")), (dict(dact=2), ("dact=2 without aux",)), (dict(dact=1), ("dact=1 without aux",)),
    (dict(QKV_FIELDS, q=0), ("QKV", "q, k, vt")), (dict(QKV_FIELDS, k=0), ("QKV", "q, k, vt")), (dict(QKV_FIELDS, vt=0), ("QKV", "q, k, vt")),
    (dict(QKV_FIELDS, T=0), ("QKV", "T=0")), (dict(QKV_FIELDS, M=170), ("QKV", "M=170", "T=40")), (dict(QKV_FIELDS, N=128, bt_rows=128), ("QKV", "N=128", "3 * H * dh")),
    (dict(QKV_FIELDS, H=0), ("QKV", "H=0")), (dict(QKV_FIELDS, vt=32772), ("misaligned vt",)),
    (dict(QKV_FIELDS, T=20), ("gemm_nt: QKV split needs T, dh multiples of 8",)), (dict(QKV_FIELDS, dh=12, H=4, N=144), ("gemm_nt: QKV split needs",)),
    (dict(M=0), ("gemm_nt: bad shape",)), (dict(N=-4), ("gemm_nt: bad shape",)), (dict(K=0), ("gemm_nt: bad shape",)),
    (dict(K=12), ("gemm_nt: A rows must be 16-byte aligned",)), (dict(dtA=F32, dtM=F32, dtC=F32, K=6), ("gemm_nt: A rows must be 16-byte aligned",)),
    (dict(dtC=F32, dtM=F32), ("gemm_nt: unsupported dtype combination",)), (dict(dtA=F32, dtC=F32), ("gemm_nt: unsupported dtype combination",)),
    (dict(dtA=F16, dtM=F16, dtC=F16, op=4), ("gemm_nt: f16 operands take no operand transform",)), (dict(dtA=F16, dtM=F16, dtC=BF16), ("gemm_nt: unsupported f16 dtype combination",)),
    (dict(dtA=F32, dtM=BF16, dtC=BF16, op=1), ("gemm_nt: unsupported dtype combination",)),
    (dict(M=34816, N=768, K=640, bt_rows=768, ldb=640), ("route NT_BIG", "only the tile kernels")),
]


@pytest.mark.parametrize("kw,words", GEMM_NT_REFUSALS)
def test_gemm_nt_refuses_buffers_dtypes_and_shapes(lib, kw, words):
    _refused(lib, _gemm_nt(lib, **kw), "ishara_op_gemm_nt", *words)
    rc, route, kernel = _gemm_nt_route(lib, **kw)
    assert (rc, route, kernel) == (0, b"NT_REFUSED", b"")
    _refused(lib, -1, "ishara_debug_gemm_nt_route", *words)


def test_gemm_nt_null_arguments_and_accepted_calls(lib):
    _refused(lib, lib.ishara_op_gemm_nt(None, N), "ishara_op_gemm_nt", "null call")
    route, kernel = C.c_char_p(), C.c_char_p()
    k = _gemm_nt_call()
    _refused(lib, lib.ishara_debug_gemm_nt_route(None, C.byref(route), C.byref(kernel)), "ishara_debug_gemm_nt_route", "null")
    _refused(lib, lib.ishara_debug_gemm_nt_route(C.byref(k), None, C.byref(kernel)), "ishara_debug_gemm_nt_route", "null")
    _refused(lib, lib.ishara_debug_gemm_nt_route(C.byref(k), C.byref(route), None), "ishara_debug_gemm_nt_route", "null")
    # what the refusal rows vary, unvaried, is taken: each row is refused for its own field
    assert _gemm_nt_route(lib) == (0, b"NT_TILE_T", b"gemm_nt_t_kernel<bf16,bf16>")
    assert _gemm_nt_route(lib, **QKV_FIELDS) == (0, b"NT_TILE_T", b"gemm_nt_t_kernel<bf16,bf16>")
    assert _gemm_nt_route(lib, C=12296) == (0, b"NT_TILE_T", b"gemm_nt_t_kernel<bf16,bf16>")          # 8-byte aligned 16-bit C: the 128 x 128 kernel stores 4 elements
    assert _gemm_nt_route(lib, N=130, bt_rows=256) == (0, b"NT_GLDS", b"gemm_nt_glds_kernel<bf16,bf16>")
    _refused(lib, _gemm_nt(lib, N=130, C=12296), "ishara_op_gemm_nt", "misaligned C", "16-byte", "NT_GLDS")
    assert _gemm_nt_route(lib, K=72, ldb=128) == (0, b"NT_REG", b"gemm_nt_kernel<bf16,bf16,bf16>")
    assert _gemm_nt_route(lib, addtab=40964, K=72, ldb=128) == (0, b"NT_REG", b"gemm_nt_kernel<bf16,bf16,bf16>")      # 4-byte aligned table off the 128 x 128 kernel
    try:      # the switches steer the answer, as they steer the launcher
        lib.ishara_debug_force_regstage(8)
        assert _gemm_nt_route(lib)[1] == b"NT_GLDS"
        lib.ishara_debug_force_regstage(1)
        assert _gemm_nt_route(lib)[1] == b"NT_REG"
        lib.ishara_debug_force_regstage(8192)
        assert _gemm_nt_route(lib, M=34816, N=768, K=640, bt_rows=768, ldb=640)[1] == b"NT_TILE_T"
    finally:
        lib.ishara_debug_force_regstage(0)


# ---- ishara_op_gemm_as / ishara_debug_gemm_as_plan: what ishara_op_gemm_nt refuses, plus the fields only the A-stationary family reads; a call
# that lands on another kernel is refused by the route's name.  The plan entry answers "NT_REFUSED", everything else zero, with the same message
AS_EXT = ("ln_gamma", "ln_beta", "ln_mean", "ln_rstd", "pa_P", "pa_Q", "pro_out", "ln_eps", "ldc", "n_valid", "as_flags")


def _gemm_as_call(**kw):
    """(call, ext): a plain bf16 call of the per-step kernel (K = 256, bias + residual, 64-row workgroups) with made-up aligned addresses, `kw`
    replacing single fields of either struct"""
    v = dict(M=200, N=96, K=256, bt_rows=96, ldb=256)
    v.update({n: x for n, x in kw.items() if n not in AS_EXT})
    k, x = _gemm_nt_call(**v), _lib.GemmAsExt()
    for n, val in dict(dict(as_flags=51, ln_eps=1e-5), **{n: x for n, x in kw.items() if n in AS_EXT}).items():
        setattr(x, n, val)
    return k, x


def _gemm_as(L, **kw):
    k, x = _gemm_as_call(**kw)
    return L.ishara_op_gemm_as(C.byref(k), C.byref(x), N)


def _gemm_as_plan(L, **kw):
    k, x = _gemm_as_call(**kw)
    p = _lib.GemmAsPlan()
    rc = L.ishara_debug_gemm_as_plan(C.byref(k), C.byref(x), C.byref(p))
    return rc, p


LN_FIELDS = dict(ln_gamma=40960, ln_beta=45056, resid=0)
PA_FIELDS = dict(pa_P=40960, pa_Q=45056, T=64)
AS_QKV = dict(mode=1, q=24576, k=28672, vt=32768, C=0, resid=0, T=40, H=1, dh=32, M=160)
GEMM_AS_REFUSALS = [
    # what the tile entry refuses too
    (dict(dtA=5), ("unknown dtype", "dtA=5")), (dict(op=5), ("unknown op=5",)), (dict(act=3), ("unknown act=3",)), (dict(dact=3), ("unknown dact=3",)),
    (dict(mode=2), ("unknown mode=2",)), (dict(head_major=2), ("head_major=2",)), (dict(rowscale_bias=2), ("rowscale_bias=2",)), (dict(drop_rate=1.0), ("drop_rate",)),
    (dict(A=0), ("null A",)), (dict(Bt=0), ("null Bt",)), (dict(C=0), ("null C",)), (dict(Bt=8200), ("misaligned Bt",)), (dict(A=4104), ("gemm_nt: A rows must be 16-byte aligned",)),
    (dict(addtab=40960, tab_period=0), ("tab_period=0",)), (dict(rowscale=40960, T=0), ("rowscale", "T=0")), (dict(dact=2), ("dact=2 without aux",)),
    (dict(AS_QKV, q=0), ("QKV", "q, k, vt")), (dict(AS_QKV, M=170), ("QKV", "M=170")), (dict(AS_QKV, N=64, bt_rows=64), ("QKV", "N=64")),
    (dict(AS_QKV, T=20), ("gemm_nt: QKV split needs T, dh multiples of 8",)), (dict(M=0), ("gemm_nt: bad shape",)),
    # the weight shadow of this family
    (dict(bt_rows=95), ("bt_rows=95", "N=96")), (dict(bt_rows=0), ("bt_rows=0",)), (dict(ldb=192), ("ldb=192", "K=256")), (dict(ldb=288), ("ldb=288", "multiple of 64")),
    # outputs and side operands: 16 bytes
    (dict(C=12296), ("misaligned C", "16-byte")), (dict(resid=20488), ("misaligned resid", "16-byte")), (dict(pre_out=40968), ("misaligned pre_out",)),
    (dict(dact=2, aux=40968, resid=0), ("misaligned aux",)), (dict(addtab=40964, resid=0), ("misaligned addtab", "16-byte")), (dict(AS_QKV, q=24584), ("misaligned q",)),
    (dict(AS_QKV, k=28680), ("misaligned k",)), (dict(AS_QKV, vt=32769), ("misaligned vt",)), (dict(LN_FIELDS, pro_out=49160), ("misaligned pro_out", "16-byte")),
    (dict(bias=16386), ("misaligned bias", "4-byte")), (dict(LN_FIELDS, ln_gamma=40962), ("misaligned ln_gamma",)), (dict(LN_FIELDS, ln_mean=49154, ln_rstd=53248), ("misaligned ln_mean",)),
    (dict(PA_FIELDS, pa_Q=45058), ("misaligned pa_Q",)),
    # the ext's own fields
    (dict(as_flags=-2), ("as_flags=-2",)), (dict(as_flags=512), ("as_flags=512",)),
    (dict(LN_FIELDS, pa_P=49152, pa_Q=53248), ("ln_gamma and pa_P",)), (dict(ln_gamma=40960, resid=0), ("ln_gamma and ln_beta",)), (dict(pa_Q=45056), ("pa_P and pa_Q",)),
    (dict(LN_FIELDS, ln_mean=49152), ("ln_mean and ln_rstd",)), (dict(ln_mean=49152, ln_rstd=53248), ("ln_mean / ln_rstd without ln_gamma",)),
    (dict(pro_out=49152), ("pro_out without a prologue",)), (dict(LN_FIELDS, ln_eps=-1.0), ("ln_eps",)), (dict(LN_FIELDS, ln_eps=float("nan")), ("ln_eps",)),
    # a prologue run_as has no instantiation for: the epilogue mask, the C type, K
    (dict(LN_FIELDS, resid=20480), ("ln_gamma", "LayerNorm", "mask 1", "no instantiation")), (dict(LN_FIELDS, act=2), ("ln_gamma", "mask 4")),
    (dict(PA_FIELDS, resid=0), ("pa_P", "affine", "mask 0", "no instantiation")), (dict(PA_FIELDS, act=2), ("pa_P", "mask 5")),
    (dict(LN_FIELDS, dtC=F32), ("ln_gamma", "dtC=0", "no instantiation")), (dict(LN_FIELDS, dtA=F16, dtM=F16, dtC=F32), ("ln_gamma", "dtC=0")),
    (dict(LN_FIELDS, dtA=F16, dtM=F16, dtC=F16, resid=20480), ("ln_gamma", "mask 1")), (dict(LN_FIELDS, K=128, ldb=128), ("ln_gamma", "K=128")),
    # pa_P: a workgroup's rows inside one sample
    (dict(PA_FIELDS, T=0), ("pa_P", "T=0")), (dict(PA_FIELDS, T=96), ("pa_P", "T=96", "64 rows per workgroup")), (dict(PA_FIELDS, T=64, M=1600), ("pa_P", "T=64", "128 rows per workgroup")),
    (dict(PA_FIELDS, T=128, M=33000, K=512, ldb=512), ("pa_P", "T=128", "192 rows per workgroup")), (dict(PA_FIELDS, dtA=F16, dtM=F16, dtC=F16, T=96), ("pa_P", "T=96")),
    # the narrow output
    (dict(ldc=-8), ("ldc=-8",)), (dict(ldc=88, resid=0), ("ldc=88", "columns a row stores")), (dict(ldc=100, resid=0), ("ldc=100", "16-byte")), (dict(dtC=F32, ldc=98, resid=0), ("ldc=98", "16-byte")),
    (dict(n_valid=-8), ("n_valid=-8",)), (dict(n_valid=104, resid=0), ("n_valid=104", "N=96")), (dict(n_valid=60, resid=0), ("n_valid=60", "store group", "8 columns")),
    (dict(dtC=F32, n_valid=62, resid=0), ("n_valid=62", "4 columns")), (dict(n_valid=56, ldc=48, resid=0), ("ldc=48",)),
    (dict(n_valid=88), ("n_valid=88", "resid")), (dict(ldc=104), ("ldc=104", "resid")), (dict(ldc=104, resid=0, dact=2, aux=40960), ("ldc=104", "aux")),
    (dict(AS_QKV, n_valid=88), ("n_valid=88", "QKV")),
    # calls that land on another kernel: by the route's name
    (dict(K=64, ldb=64), ("route NT_TILE_T", "only the A-stationary kernels")), (dict(N=98, bt_rows=98), ("route NT_GLDS", "only the A-stationary kernels")),
    (dict(N=1056, bt_rows=1056, resid=0), ("route NT_TILE_T",)), (dict(M=49536, N=256, K=512, bt_rows=256, ldb=512, as_flags=115), ("route NT_CS", "bits 6 / 7")),
    (dict(M=32768, N=512, K=512, bt_rows=512, ldb=512), ("route NT_BIG",)), (dict(dtA=F32, dtM=F32, dtC=F32), ("route NT_TILE_T",)),
    (dict(dtA=F16, dtM=F16, dtC=F16, K=128, ldb=128), ("route NT_REG",)), (dict(op=1), ("route NT_REG",)), (dict(dtA=F32), ("route NT_REG",)),
]


@pytest.mark.parametrize("kw,words", GEMM_AS_REFUSALS)
def test_gemm_as_refuses_fields_prologues_and_other_routes(lib, kw, words):
    _refused(lib, _gemm_as(lib, **kw), "ishara_op_gemm_as", *words)
    rc, p = _gemm_as_plan(lib, **kw)
    assert (rc, p.route, p.kernel) == (0, b"NT_REFUSED", b"")
    assert (p.rows, p.gx, p.gy, p.nsteps, p.ring, p.cs, p.waves, p.passes, tuple(p.pass_rows), p.chunked, p.hold, p.inst_mask, p.prologue) == (0,) * 8 + ((0, 0),) + (0,) * 4
    _refused(lib, -1, "ishara_debug_gemm_as_plan", *words)


def test_gemm_as_null_arguments_and_accepted_calls(lib):
    k, x = _gemm_as_call()
    p = _lib.GemmAsPlan()
    _refused(lib, lib.ishara_op_gemm_as(None, C.byref(x), N), "ishara_op_gemm_as", "null call")
    _refused(lib, lib.ishara_op_gemm_as(C.byref(k), None, N), "ishara_op_gemm_as", "null ext")
    for args in ((None, C.byref(x), C.byref(p)), (C.byref(k), None, C.byref(p)), (C.byref(k), C.byref(x), None)):
        _refused(lib, lib.ishara_debug_gemm_as_plan(*args), "ishara_debug_gemm_as_plan", "null")

    def plan(**kw):
        rc, p = _gemm_as_plan(lib, **kw)
        assert rc == 0, lib.ishara_last_error()
        return p.route, p.kernel, p.rows, p.gx, p.gy, p.nsteps, p.inst_mask, p.prologue

    # what the refusal rows vary, unvaried, is taken: each row is refused for its own field
    assert plan() == (b"NT_AS", b"gemm_nt_as_kernel<bf16,8,1,0>", 64, 4, 1, 3, 1, 0)
    assert plan(**LN_FIELDS) == (b"NT_AS", b"gemm_nt_as_kernel<bf16,8,0,0,1>", 64, 4, 1, 3, 0, 1)
    assert plan(**LN_FIELDS, ln_mean=49152, ln_rstd=53248, pro_out=57344)[0] == b"NT_AS"
    assert plan(**PA_FIELDS) == (b"NT_AS", b"gemm_nt_as_kernel<bf16,8,1,0,2>", 64, 4, 1, 3, 1, 2)
    assert plan(**PA_FIELDS, dtA=F16, dtM=F16, dtC=F16) == (b"NT_AS_F16", b"gemm_nt_kernel<f16>", 64, 4, 1, 3, 1, 2)
    assert plan(**AS_QKV)[:2] == (b"NT_AS", b"gemm_nt_as_kernel<bf16,8,64,0>")
    assert plan(**dict(AS_QKV, vt=32770))[0] == b"NT_AS"                                 # vt takes single elements
    assert plan(dtC=F32, n_valid=60, ldc=60, resid=0, N=64, bt_rows=64)[:2] == (b"NT_AS", b"gemm_nt_as_kernel<f32,8,0,0>")      # the classifier's call
    assert plan(n_valid=56, ldc=72, resid=0, N=64, bt_rows=64)[0] == b"NT_AS"
    assert plan(ldb=320)[0] == b"NT_AS" and plan(bt_rows=4096)[0] == b"NT_AS"
    assert plan(as_flags=-1)[0] == b"NT_AS"
    assert plan(M=49536, N=256, K=512, bt_rows=256, ldb=512)[:3] == (b"NT_AS", b"gemm_nt_as_chunk_kernel<bf16,16,1,0>", 384)      # without bits 6 / 7
    try:      # a forced tile kernel takes the call away from the family, as it does in the launcher
        lib.ishara_debug_force_regstage(8192)
        _refused(lib, _gemm_as(lib), "ishara_op_gemm_as", "route NT_TILE_T")
    finally:
        lib.ishara_debug_force_regstage(0)
