"""GPU: the fp16 (ISHARA_F16) inference kernels, operator by operator, against torch fp64 on the same fp16-rounded inputs.

Every case lands on one kernel route (named in its id: `as` / `tile` A-stationary or tile GEMM, `stream` / `reg8` / `reg` / `tile` depthwise
conv, `mfma` / `valu` attention, classifier routes 1-3).  Tolerances come from fp16's unit roundoff u = 2^-11 and the fp16 roundings on the
kernel's path (stated per test): an element passes when |got - ref| <= R*u*|ref| + A*u*scale.  Every fp16 test also checks that its tolerance
REJECTS the fp64 reference rounded through bf16 — every fp16 rounding on the kernel's path (the output; where the path has one, the MFMA
operand it rounds: attention's P, the LayerNorm output in front of the QKV GEMM) done in bf16 instead — on a material fraction of the
elements, i.e. that it tells fp16 arithmetic from bf16 arithmetic (a kernel that converted through bf16, or ran a bf16 MFMA on fp16 data,
would pass a bf16 tolerance).  Observed errors are logged with test_model_gpu's _log_observed."""
import ctypes as C
import zlib

import pytest
import torch
import torch.nn.functional as F

from ishara_amd import _lib
from test_model_gpu import _log_observed

pytestmark = pytest.mark.gpu

F32, BF16, F16 = _lib.F32, _lib.BF16, _lib.F16
U16 = 2.0 ** -11            # fp16 unit roundoff
UBF = 2.0 ** -8             # bf16 unit roundoff
BF16_REJECT_MIN = 0.10      # the tolerance must reject the bf16-rounded reference on at least this fraction of the elements


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def scratch(nbytes):
    """(tensor, 256-byte aligned pointer) of at least nbytes"""
    sc = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device="cuda")
    return sc, C.c_void_p(sc.data_ptr() + (-sc.data_ptr()) % 256)


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def randn(g, *shape, std=1.0, mean=0.0):
    return (torch.randn(*shape, generator=g) * std + mean).cuda()


def check(name, got, ref, R, A, scale=None, u=U16, bf16_reject=True, bf16_ref=None, **info):
    """|got - ref| <= R*u*|ref| + A*u*scale elementwise (scale: rms of ref unless given; a number or a tensor of ref's shape); with bf16_reject,
    the same bound must reject bf16_ref (default: ref rounded to bf16) on >= BF16_REJECT_MIN of the elements"""
    got, ref = got.detach().double(), ref.detach().double().to(got.device)
    scale = float(ref.pow(2).mean().sqrt()) if scale is None else (scale.double().to(ref.device) if torch.is_tensor(scale) else float(scale))
    tol = R * u * ref.abs() + A * u * scale
    err = (got - ref).abs()
    ratio = float((err / tol).max())
    rec = dict(test="ops_f16", op=name, **info, max_abs_err=float(err.max()), ref_scale=float(ref.abs().max()), scale=float(scale.max()) if torch.is_tensor(scale) else scale,
               R=R, A=A, u=u, err_over_tol=ratio)
    frac = None
    if bf16_reject:
        rb = (ref.to(torch.bfloat16) if bf16_ref is None else bf16_ref.to(ref.device)).double()
        frac = float(((rb - ref).abs() > tol).double().mean())
        rec["bf16_rejected_frac"] = frac
    _log_observed(rec)
    assert ratio <= 1.0, f"{name} {info}: max abs err {float(err.max()):.3e} is {ratio:.2f}x the tolerance (R={R}u |ref| + A={A}u * scale)"
    if bf16_reject:
        assert frac >= BF16_REJECT_MIN, f"{name} {info}: the tolerance rejects the bf16-rounded reference on only {frac:.3f} of the elements"


def act_ref(z, act):
    return [z, z * torch.sigmoid(z), torch.relu(z)][act]


# ------------------------------------------------------------------ dense forward
# A-stationary fp16 kernel (gemm_as_f16.hip): K 256 / 512, N <= 1024; M on both sides of the row-form boundaries (AS_SMALL_M = 1536: 64 vs
# 128 rows at K = 256; AS_MID_M_K512 = 32768: 64 vs 192 rows at K = 512).  Output rounding to fp16 (<= u |y|) is the only fp16 rounding
# (f16 x f16 products are exact in fp32, fp32 accumulation): R = 2, A = 1/4 (accumulation order on small outputs).
AS_M = [1, 63, 176, 384, 1536, 1537, 3000]
DENSE_AS = [pytest.param(M, K, N, (M + N // 64) % 3, (M + K // 256 + N // 64) % 2 == 0, id=f"as-K{K}-N{N}-M{M}")
            for K in (256, 512) for N in (64, 256, 512, 768, 1024) for M in AS_M]
# tile kernel (gemm_nt_kernel<f16,...>, K tile 64): K not 256 / 512 (K 96 / 288: a partial last K tile), ragged N
DENSE_TILE = [pytest.param(300 + 7 * i, K, N, i % 3, i % 2 == 0, id=f"tile-K{K}-N{N}") for i, (K, N) in enumerate(
    [(K, N) for K in (64, 96, 128, 288, 320, 1024) for N in (8, 60, 200)])]
DENSE_A = 0.25


def _dense(lib, M, K, N, act, with_resid, regstage=0, xs=1.0, ws=1.0, rows=None):
    g = _gen("dense", M, K, N, act, with_resid, xs)
    x = randn(g, M, K, std=xs).half()
    W = randn(g, K, N, std=ws / K ** 0.5)
    b = randn(g, N)
    r = randn(g, M, N, std=xs * ws).half() if with_resid else None
    y = torch.empty(M, N, dtype=torch.float16, device="cuda")
    _sc, scp = scratch(lib.ishara_op_scratch_bytes(M, K, N))
    lib.ishara_debug_force_regstage(regstage)
    try:
        _lib.check(lib.ishara_op_dense_fwd_ex(F16, _lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(r), _lib.ptr(y), M, K, N, act, scp, stream()))
        torch.cuda.synchronize()
    finally:
        lib.ishara_debug_force_regstage(0)
    if rows is None:
        rows = torch.arange(M, device="cuda")
    ref = act_ref(x[rows].double() @ W.half().double() + b.double(), act)
    if with_resid:
        ref = ref + r[rows].double()
    return y[rows], ref


@pytest.mark.parametrize("M,K,N,act,with_resid", DENSE_AS + DENSE_TILE)
def test_dense_fwd(lib, M, K, N, act, with_resid):
    y, ref = _dense(lib, M, K, N, act, with_resid)
    check("dense_fwd", y, ref, 2, DENSE_A, M=M, K=K, N=N, act=act, resid=with_resid)


@pytest.mark.parametrize("M,K,N,act,with_resid", [pytest.param(M, K, N, i % 3, i % 2 == 1, id=f"tile-forced-K{K}-N{N}-M{M}")
                                                  for i, (M, K, N) in enumerate([(176, 256, 64), (1537, 256, 512), (384, 512, 256), (3000, 512, 1024)])])
def test_dense_fwd_forced_tile(lib, M, K, N, act, with_resid):
    """K 256 / 512 on the tile kernel (ishara_debug_force_regstage(1)): the shapes the A-stationary kernel otherwise takes"""
    y, ref = _dense(lib, M, K, N, act, with_resid, regstage=1)
    check("dense_fwd", y, ref, 2, DENSE_A, M=M, K=K, N=N, act=act, resid=with_resid, route="tile-forced")


@pytest.mark.parametrize("regstage", [pytest.param(0, id="as"), pytest.param(1, id="tile")])
def test_dense_fwd_large_outputs(lib, regstage):
    """inputs scaled so that the outputs reach ~1e4 (fp16 max 65504): intermediate fp16 arithmetic would overflow or lose bits"""
    y, ref = _dense(lib, 384, 256, 256, 0, True, regstage=regstage, xs=40.0, ws=40.0)
    assert float(ref.abs().max()) > 4e3 and float(ref.abs().max()) < 6e4
    check("dense_fwd_large", y, ref, 2, DENSE_A, route="as" if regstage == 0 else "tile")


def test_dense_fwd_above_mid_m_k512(lib):
    """K = 512, M above AS_MID_M_K512 (192-row workgroups as a 128-row and a 64-row pass, ragged last workgroup): sampled rows"""
    M = 32768 + 200
    rows = torch.cat([torch.arange(0, 700), torch.arange(M // 2 - 200, M // 2 + 200), torch.arange(M - 500, M)]).cuda()
    y, ref = _dense(lib, M, 512, 512, 1, True, rows=rows)
    check("dense_fwd", y, ref, 2, DENSE_A, M=M, K=512, N=512, route="as-192")


# ------------------------------------------------------------------ LayerNorm forward
# fp32 statistics of fp16 rows, output rounded to fp16: R = 2; A covers the fp32 mean's rounding relative to a small spread (offset rows:
# the mean of values ~50 carries ~3e-5 of fp32 rounding against a spread of 0.1)
LN_A = 0.25
LN_A_OFFSET = 1.0
LN_MEAN_TOL = 1e-7
LN_RSTD_TOL = 4e-7


@pytest.mark.parametrize("offset", [pytest.param(False, id="centred"), pytest.param(True, id="mean50-std0.1")])
@pytest.mark.parametrize("M", [1, 77, 1000, 4099])
@pytest.mark.parametrize("Cc", [64, 128, 192, 256, 512])
def test_layernorm_fwd(lib, Cc, M, offset):
    g = _gen("ln", Cc, M, offset)
    x = (randn(g, M, Cc, std=0.1, mean=50.0) if offset else randn(g, M, Cc, std=2.0, mean=0.5)).half()
    gamma, beta = randn(g, Cc), randn(g, Cc)
    y = torch.empty_like(x)
    mean, rstd = torch.empty(M, device="cuda"), torch.empty(M, device="cuda")
    _lib.check(lib.ishara_op_layernorm_fwd(F16, _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), C.c_float(1e-6), _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd), M, Cc, stream()))
    torch.cuda.synchronize()
    xd = x.double()
    ref = F.layer_norm(xd, (Cc,), gamma.double(), beta.double(), 1e-6)
    check("layernorm_fwd", y, ref, 2, LN_A_OFFSET if offset else LN_A, C=Cc, M=M, offset=offset)
    mu = xd.mean(1)
    var = xd.var(1, unbiased=False)
    # fp32 statistics: observed <= 3e-8 (mean, relative to |mean| + the rows' spread) and 1.6e-7 (rstd, relative)
    check("layernorm_mean", mean, mu, LN_MEAN_TOL / U16, LN_MEAN_TOL / U16, scale=float(var.sqrt().max()), bf16_reject=False, C=Cc, M=M, offset=offset)
    check("layernorm_rstd", rstd, 1.0 / (var + 1e-6).sqrt(), LN_RSTD_TOL / U16, 0, bf16_reject=False, C=Cc, M=M, offset=offset)


# ------------------------------------------------------------------ depthwise conv forward
def _dw_ref(x, w, bias, inop, padl, C_):
    if inop == 1:
        u = x * torch.sigmoid(x)
    elif inop == 2:
        u = x[..., :C_] * torch.sigmoid(x[..., C_:])
    else:
        u = x
    k = w.shape[0]
    up = F.pad(u.transpose(1, 2), (padl, k - 1 - padl))
    return F.conv1d(up, w.t().unsqueeze(1), bias, groups=C_).transpose(1, 2)


# (route, B, T, C, k, inop, causal, stats, entry): route conditions at dwconv.hip dwconv_fwd_route
#   stream: B > 8, k 11 / 15, C % 128 == 0, T >= 64, statistics only through the caller's scratch (_ex)
#   reg8:   k 3 / 5, C / 8 in {32, 64, 128, 256}, statistics only through scratch (or none)
#   reg:    k 3 / 5, C / 4 a power of two <= 256 (the plain entry point with statistics, or C / 8 < 32)
#   tile:   everything else (k 11 / 15 at B <= 8 or without scratch, k 31, T < k) and the forced LDS-tiled kernel
DW_CASES = [
    ("stream", 9, 384, 512, 11, 1, True, True, "ex"), ("stream", 9, 200, 128, 15, 2, False, True, "ex"),
    ("stream", 12, 64, 256, 11, 0, False, True, "ex"), ("stream", 10, 100, 128, 15, 1, True, False, "ex"),
    ("reg8", 2, 384, 256, 3, 1, True, True, "ex"), ("reg8", 3, 176, 512, 5, 2, False, True, "ex"),
    ("reg8", 1, 100, 1024, 5, 0, True, False, "plain"), ("reg8", 9, 77, 256, 3, 0, False, True, "ex"),
    ("reg", 2, 176, 128, 3, 1, False, True, "plain"), ("reg", 2, 100, 64, 5, 2, True, True, "ex"),
    ("reg", 3, 384, 256, 5, 1, True, True, "plain"), ("reg", 1, 37, 32, 3, 0, False, False, "plain"),
    ("tile", 2, 176, 256, 11, 1, True, True, "plain"), ("tile", 2, 16, 512, 31, 2, False, True, "plain"),
    ("tile", 2, 100, 128, 31, 0, True, True, "ex"), ("tile", 2, 7, 128, 11, 1, True, True, "plain"),
    ("tile", 1, 7, 64, 15, 2, False, True, "ex"), ("tile", 3, 7, 256, 11, 0, False, False, "ex"),
    ("tile-forced", 9, 384, 512, 11, 1, True, True, "ex"), ("tile-forced", 2, 200, 256, 5, 2, False, False, "ex"),
]
DW_A = 0.5
DW_STATS_TOL = 1e-6


@pytest.mark.parametrize("route,B,T,Cc,k,inop,causal,stats,entry", [pytest.param(*c, id=f"{c[0]}-B{c[1]}-T{c[2]}-C{c[3]}-k{c[4]}-op{c[5]}-{'causal' if c[6] else 'same'}-{'stats' if c[7] else 'nostats'}-{c[8]}") for c in DW_CASES])
def test_dwconv_fwd(lib, route, B, T, Cc, k, inop, causal, stats, entry):
    g = _gen("dw", route, B, T, Cc, k, inop, causal)
    Cin = 2 * Cc if inop == 2 else Cc
    x = randn(g, B, T, Cin).half()
    w = randn(g, k, Cc, std=1.0 / k ** 0.5)
    bias = None if causal else randn(g, Cc)
    padl = k - 1 if causal else (k - 1) // 2
    y = torch.empty(B, T, Cc, dtype=torch.float16, device="cuda")
    ssum = torch.zeros(B, Cc, device="cuda") if stats else None
    ssq = torch.zeros(B, Cc, device="cuda") if stats else None
    lib.ishara_debug_force_regstage(4 if route == "tile-forced" else 0)
    try:
        if entry == "ex":
            _sc, scp = scratch(lib.ishara_op_dwconv_fwd_scratch_bytes(B, T, Cc))
            _lib.check(lib.ishara_op_dwconv_fwd_ex(F16, inop, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), _lib.ptr(ssum), _lib.ptr(ssq), scp, B, T, Cc, k, padl, stream()))
        else:
            _lib.check(lib.ishara_op_dwconv_fwd(F16, inop, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(y), _lib.ptr(ssum), _lib.ptr(ssq), B, T, Cc, k, padl, stream()))
        torch.cuda.synchronize()
    finally:
        lib.ishara_debug_force_regstage(0)
    ref = _dw_ref(x.double(), w.double(), bias.double() if bias is not None else None, inop, padl, Cc)
    info = dict(route=route, B=B, T=T, C=Cc, k=k, inop=inop, causal=causal, entry=entry)
    check("dwconv_fwd", y, ref, 2, DW_A, **info)
    if stats:
        # fp32 sums over T of the fp32 outputs (before their fp16 rounding): fp32 accumulation only, observed < 5e-7 of sum|y|
        refs, refq = ref.sum(1), (ref ** 2).sum(1)
        es, eq = (ssum.double() - refs).abs(), (ssq.double() - refq).abs()
        bs, bq = DW_STATS_TOL * ref.abs().sum(1) + 1e-7, DW_STATS_TOL * (ref ** 2).sum(1) + 1e-7
        _log_observed(dict(test="ops_f16", op="dwconv_stats", **info, ssum_err_over_tol=float((es / bs).max()), ssq_err_over_tol=float((eq / bq).max())))
        assert bool((es <= bs).all()), f"ssum: {float((es / bs).max()):.2f}x the bound"
        assert bool((eq <= bq).all()), f"ssq: {float((eq / bq).max()):.2f}x the bound"


# ------------------------------------------------------------------ attention forward
def _attn_ref(qkv, B, H, T, dh, scale):
    q4 = qkv.view(B, T, H, 3 * dh).permute(0, 2, 1, 3)
    q, k, v = q4[..., :dh], q4[..., dh:2 * dh], q4[..., 2 * dh:]
    a = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    return (a @ v).permute(0, 2, 1, 3).reshape(B * T, H * dh)


# impl 1 + fp16: the MFMA flash kernel (attn_fwd_mfma_kernel<dh,0,f16>) when dh is 32 / 64 and T % 8 == 0 — P is rounded to fp16 for the
# P.V product, a random walk of u * s per output, s = sqrt(sum_j a_j^2 v_j^2) (a the softmax row): A = 2.5 times that elementwise s (the
# tail of up to 1e6 outputs); else the VALU kernel attn_fwd_kernel<f16> with fp32 P: only the output rounding, A = 1/4 of unit-variance v
ATT_CASES = ([pytest.param(1, 2, 64 // dh * 2, T, dh, sharp, id=f"mfma-dh{dh}-T{T}-x{sharp}") for dh in (32, 64) for T in (8, 176, 200, 384, 512) for sharp in (4, 16)]
             + [pytest.param(1, 2, 2, T, dh, 4, id=f"valu-fallback-dh{dh}-T{T}") for dh in (32, 64) for T in (1, 37, 100)]
             + [pytest.param(0, 2, 4, 176 if dh % 16 else 100, dh, sharp, id=f"valu-dh{dh}-x{sharp}") for dh in (8, 16, 24, 32, 48, 64) for sharp in (4, 16)])
ATT_A_MFMA = 2.5
ATT_A_VALU = 0.25


def _attn_walk(qkv, B, H, T, dh, scale):
    """s = sqrt(sum_j a_j^2 v_j^2) per output element, the scale of the error that rounding P contributes"""
    q4 = qkv.view(B, T, H, 3 * dh).permute(0, 2, 1, 3)
    q, k, v = q4[..., :dh], q4[..., dh:2 * dh], q4[..., 2 * dh:]
    a = torch.softmax(q @ k.transpose(-1, -2) * scale, -1)
    return ((a * a) @ (v * v)).sqrt().permute(0, 2, 1, 3).reshape(B * T, H * dh)


def _attn_bf16_path(qkv, B, H, T, dh, scale, mfma):
    """the reference with the MFMA path's roundings done in bf16: P (before the P.V product) and the output"""
    if not mfma:
        return None
    q4 = qkv.view(B, T, H, 3 * dh).permute(0, 2, 1, 3)
    q, k, v = q4[..., :dh], q4[..., dh:2 * dh], q4[..., 2 * dh:]
    s = q @ k.transpose(-1, -2) * scale
    p = torch.exp(s - s.amax(-1, keepdim=True))
    o = (p.to(torch.bfloat16).double() @ v) / p.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B * T, H * dh).to(torch.bfloat16)


def _attn_run(lib, B, H, T, dh, scale, impl, g):
    d = H * dh
    qkv = randn(g, B * T, 3 * d).half()
    o = torch.empty(B * T, d, dtype=torch.float16, device="cuda")
    _sc, scp = scratch(lib.ishara_op_attn_scratch_bytes(B, H, T, dh))
    _lib.check(lib.ishara_op_attn_fwd(F16, _lib.ptr(qkv), _lib.ptr(o), B, H, T, dh, C.c_float(scale), 0, 0, C.c_float(0.0), impl, scp, stream()))
    torch.cuda.synchronize()
    return qkv, o


@pytest.mark.parametrize("impl,B,H,T,dh,sharp", ATT_CASES)
def test_attention_fwd(lib, impl, B, H, T, dh, sharp):
    scale = (H * dh) ** -0.5 * sharp        # x4 / x16 the model's dim ** -0.5: a sharper softmax exercises the running-max rescaling
    qkv, o = _attn_run(lib, B, H, T, dh, scale, impl, _gen("attn", impl, T, dh, sharp))
    ref = _attn_ref(qkv.double(), B, H, T, dh, scale)
    mfma = impl == 1 and T % 8 == 0
    check("attn_fwd", o, ref, 2, ATT_A_MFMA if mfma else ATT_A_VALU, scale=_attn_walk(qkv.double(), B, H, T, dh, scale) if mfma else 1.0,
          bf16_ref=_attn_bf16_path(qkv.double(), B, H, T, dh, scale, mfma),
          impl=impl, B=B, H=H, T=T, dh=dh, sharp=sharp, route="mfma" if mfma else "valu")


def test_attention_fwd_batched_inference(lib):
    """B = 64, H = 8, T = 384, dh = 32 (BatchedTFLiteModel at configs[4]): 16 sampled (b, h) pairs"""
    B, H, T, dh = 64, 8, 384, 32
    scale = (H * dh) ** -0.5
    g = _gen("attn-batched")
    qkv, o = _attn_run(lib, B, H, T, dh, scale, 1, g)
    pairs = [(int(b), int(h)) for b, h in zip(torch.randint(0, B, (16,), generator=g), torch.randint(0, H, (16,), generator=g))] + [(0, 0), (B - 1, H - 1)]
    q3 = qkv.view(B, T, H, 3, dh)
    o3 = o.view(B, T, H, dh)
    got = torch.stack([o3[b, :, h] for b, h in pairs])
    ref = torch.stack([_attn_ref(q3[b, :, h].reshape(T, 3 * dh).double(), 1, 1, T, dh, scale) for b, h in pairs])
    rb = torch.stack([_attn_bf16_path(q3[b, :, h].reshape(T, 3 * dh).double(), 1, 1, T, dh, scale, True) for b, h in pairs])
    walk = torch.stack([_attn_walk(q3[b, :, h].reshape(T, 3 * dh).double(), 1, 1, T, dh, scale) for b, h in pairs])
    check("attn_fwd", got, ref, 2, ATT_A_MFMA, scale=walk, bf16_ref=rb, impl=1, B=B, H=H, T=T, dh=dh, sharp=1, route="mfma")


# ------------------------------------------------------------------ QKV projection (LayerNorm + GEMM + EPI_QKV scatter)
# R = 2 for the output rounding.  Without the LayerNorm x is the (exact) operand: A = 1/4 as the dense forward.  With it, the LayerNorm output
# is an fp16 (bf16) MFMA operand, fused or not: each of the K operand elements is rounded once, a random walk of ~u * rms(y) per output
# element that reaches ~4u in the tail of 10^7 outputs (observed 3.7u): A = 5, i.e. 5u of the outputs' rms (~1u of their max)
QKV_A = 0.25
QKV_A_LN = 5.0
QKV_CASES = ([pytest.param(dt, ln, H, dh, B, T, 1, id=f"{'f16' if dt == F16 else 'bf16'}-{'ln' if ln else 'noln'}-H{H}-dh{dh}-B{B}-T{T}")
              for dt in (F16, BF16) for ln in (True, False) for H, dh in ((4, 32), (8, 32), (8, 64)) for B, T in ((1, 176), (3, 200), (64, 384))]
             + [pytest.param(BF16, ln, H, dh, 3, 200, 0, id=f"bf16-{'ln' if ln else 'noln'}-H{H}-dh{dh}-plain-major") for ln in (True, False) for H, dh in ((4, 32), (8, 64))])


@pytest.mark.parametrize("dt,ln,H,dh,B,T,head_major", QKV_CASES)
def test_qkv_fwd(lib, dt, ln, H, dh, B, T, head_major):
    tdt = torch.float16 if dt == F16 else torch.bfloat16
    u = U16 if dt == F16 else UBF
    d, M = H * dh, B * T
    g = _gen("qkv", dt, ln, H, dh, B, T, head_major)
    x = randn(g, M, d, std=1.5, mean=0.3).to(tdt)
    gamma, beta = (randn(g, d, std=0.2, mean=1.0), randn(g, d, std=0.1)) if ln else (None, None)
    W = randn(g, d, 3 * d, std=1.0 / d ** 0.5)
    bias = randn(g, 3 * d, std=0.1)
    q = torch.empty(B, H, T, dh, dtype=tdt, device="cuda")
    k = torch.empty_like(q)
    vt = torch.empty(B, H, dh, T, dtype=tdt, device="cuda")
    _sc, scp = scratch(lib.ishara_op_qkv_scratch_bytes(B, T, H, dh))
    _lib.check(lib.ishara_op_qkv_fwd(dt, _lib.ptr(x), _lib.ptr(gamma), _lib.ptr(beta), C.c_float(1e-6), _lib.ptr(W), _lib.ptr(bias),
                                     _lib.ptr(q), _lib.ptr(k), _lib.ptr(vt), B, T, H, dh, head_major, scp, stream()))
    torch.cuda.synchronize()
    xn = x.double()
    if ln:
        xn = F.layer_norm(xn, (d,), gamma.double(), beta.double(), 1e-6)
    y = xn @ W.to(tdt).double() + bias.double()
    # bf16 path: the LayerNorm output (the operand) rounded to bf16, bf16 weights, output rounded to bf16
    yb = ((xn.to(torch.bfloat16).double() if ln else xn) @ W.to(torch.bfloat16).double() + bias.double()).to(torch.bfloat16)
    info = dict(dt=dt, ln=ln, H=H, dh=dh, B=B, T=T, head_major=head_major)

    def split(t):
        t5 = t.view(B, T, H, 3, dh) if head_major else t.view(B, T, 3, H, dh).permute(0, 1, 3, 2, 4)
        return t5[:, :, :, 0].permute(0, 2, 1, 3), t5[:, :, :, 1].permute(0, 2, 1, 3), t5[:, :, :, 2].permute(0, 2, 3, 1)
    for name, got, ref, rb in zip(("q", "k", "vt"), (q, k, vt), split(y), split(yb)):
        check(f"qkv_fwd.{name}", got, ref, 2, QKV_A_LN if ln else QKV_A, u=u, bf16_reject=dt == F16, bf16_ref=rb if dt == F16 else None, **info)


# ------------------------------------------------------------------ classifier (fp32 logits)
# f16 x f16 (bf16 x bf16) products are exact in fp32: the only error is fp32 accumulation -> ~1e-5 absolute at unit-scale logits
CLS_M = [1, 63, 65, 176, 384, 1536, 1537, 4096, 4097]
CLS_TOL = 4e-6              # observed 1.9e-6 (dense_narrow), 0.8e-6 (A-stationary, GEMM)
SENTINEL = 12345.0


def _route_takes(route, K, Cc):
    if route == 1:
        return Cc <= 64 and Cc % 4 == 0 and K in (256, 512)
    if route == 2:
        return Cc <= 64 and K % 32 == 0
    return K % 8 == 0


def _rule(M, K, Cc):
    """the documented route-0 rule (include/ishara_hip.h) for 16-bit dt"""
    if M <= 1536 and _route_takes(1, K, Cc):
        return 1
    if M <= 4096 and _route_takes(2, K, Cc):
        return 2
    return 3


@pytest.mark.parametrize("M", CLS_M)
@pytest.mark.parametrize("K,Cc", [(K, Cc) for K in (128, 256, 512) for Cc in (8, 60, 64)])
@pytest.mark.parametrize("dt", [pytest.param(F16, id="f16"), pytest.param(BF16, id="bf16")])
def test_classifier_routes(lib, dt, K, Cc, M):
    tdt = torch.float16 if dt == F16 else torch.bfloat16
    g = _gen("cls", dt, K, Cc, M)
    x = randn(g, M, K).to(tdt)
    W = randn(g, K, Cc, std=1.0 / K ** 0.5)
    b = randn(g, Cc, std=0.1)
    ref = x.double() @ W.to(tdt).double() + b.double()
    _sc, scp = scratch(lib.ishara_op_scratch_bytes(M, K, Cc))
    outs = {}
    for route in (0, 1, 2, 3):
        out = torch.full((M * Cc + 512,), SENTINEL, device="cuda")
        rc = lib.ishara_op_classifier_fwd(dt, _lib.ptr(x), _lib.ptr(W), _lib.ptr(b), _lib.ptr(out), M, K, Cc, route, scp, stream())
        torch.cuda.synchronize()
        if route and not _route_takes(route, K, Cc):
            assert rc != 0 and b"does not take" in lib.ishara_last_error(), f"route {route} accepted K={K} C={Cc}"
            assert bool((out == SENTINEL).all()), f"refused route {route} wrote its output"
            continue
        _lib.check(rc, f"classifier route {route}")
        assert bool((out[M * Cc:] == SENTINEL).all()), f"route {route} wrote past the M*C logits"
        outs[route] = out[:M * Cc].view(M, Cc)
        if route:
            check("classifier", outs[route], ref, CLS_TOL / U16, CLS_TOL / U16, scale=1.0, bf16_reject=False, dt=dt, K=K, C=Cc, M=M, route=route)
    named = _rule(M, K, Cc)
    assert torch.equal(outs[0], outs[named]), f"route 0 differs from route {named}, the one the documented rule names"
    taken = sorted(r for r in outs if r)
    for r in taken[1:]:
        d = (outs[r].double() - outs[taken[0]].double()).abs()
        assert float(d.max()) <= 2 * CLS_TOL * (1 + float(ref.abs().max())), f"routes {taken[0]} and {r} disagree by {float(d.max()):.3e}"
