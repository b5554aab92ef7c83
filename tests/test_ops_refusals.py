"""CPU: every single-operator entry point refuses what it has no kernel for — unknown dtypes, ISHARA_F16 for the backward operators (fp16
is inference-only), fp16 attention with dropout, classifier routes that do not take the shape — with an error and an ishara_last_error()
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
        "ishara_op_attn_fwd": lambda L, dt: L.ishara_op_attn_fwd(dt, N, N, 1, 4, 64, 32, f(0.1), 1, 2, f(0.0), 1, N, N),
        "ishara_op_attn_bwd": lambda L, dt: L.ishara_op_attn_bwd(dt, N, N, N, 1, 4, 64, 32, f(0.1), 1, 2, f(0.0), 1, N, N),
        "ishara_op_qkv_fwd": lambda L, dt: L.ishara_op_qkv_fwd(dt, N, N, N, f(1e-6), N, N, N, N, N, 1, 64, 4, 32, 1, N, N),
        "ishara_op_classifier_fwd": lambda L, dt: L.ishara_op_classifier_fwd(dt, N, N, N, N, 64, 256, 60, 0, N, N),
    }


BACKWARD = ["ishara_op_dense_bwd", "ishara_op_layernorm_bwd", "ishara_op_dwconv_bwd", "ishara_op_attn_bwd"]


def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the operator's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


def test_every_dtype_taking_operator_is_listed():
    """every ishara_op_* with a dtype argument (first argument) is covered below"""
    with_dt = {n for n, (_, args) in _lib.SIGNATURES.items() if n.startswith("ishara_op_") and not n.endswith("_bytes")
               and not n.startswith("ishara_op_log_softmax")}
    assert with_dt == set(_ops())


@pytest.mark.parametrize("dt", BAD_DT)
@pytest.mark.parametrize("name", sorted(_ops()))
def test_unknown_dtype_is_refused(lib, name, dt):
    _refused(lib, _ops()[name](lib, dt), name, "unknown dtype", str(dt))


@pytest.mark.parametrize("name", BACKWARD)
def test_backward_operators_refuse_f16(lib, name):
    _refused(lib, _ops()[name](lib, F16), name, "ISHARA_F16", "inference-only")


def test_f16_attention_refuses_dropout(lib):
    rc = lib.ishara_op_attn_fwd(F16, N, N, 1, 4, 64, 32, C.c_float(0.1), 1, 2, C.c_float(0.1), 1, N, N)
    _refused(lib, rc, "ishara_op_attn_fwd", "dropout")


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
