"""The K = 768 instantiation of the C-stationary GEMM (gemm_cs.hip, gemm_nt_cs_kernel<0,0,12>: the QKV projection's dgrad at training-size M),
forced at small row counts with as_flags 3 | 64 | 128 as tests/test_gemm_cs_gpu.py forces the K = 512 ones: the edges of the 256 + 128 row
split against fp64, an exact integer case, one case per 32-k half of each of the 12 K chunks (a dropped or doubled stage, a wrong S % 3 chunk
buffer or S % 4 ring slot), the route with its row threshold and off switch (as_flags bit 256), and the MHSA module at B = 2 on the route."""
import ctypes as C

import numpy as np
import pytest
import torch

import module_parity as MP
import test_gemm_cs_gpu as CS
import test_modules_gpu as TM
from ishara_amd import _lib
from test_ops_gpu import DT, TOL, close, dev, stream

pytestmark = pytest.mark.gpu

FORCED = 3 | 64 | 128
OFF = 256                 # as_flags bit 8: K = 768 stays on the 128 x 128 tile kernel
K, N = 768, 256
NEW = "gemm_nt_cs_kernel<0,0,12>"
TILE = "gemm_nt_t_kernel<bf16,bf16>"


def _dense(lib, flags, x, W, b):
    """y = x . W + b through ishara_op_dense_fwd_ex under as_flags `flags`, 8 NaN guard rows behind the output"""
    code, tdt = DT["bf16"]
    M = x.shape[0]
    xd, Wd, bd = x.cuda().contiguous(), dev(W), dev(b)
    sc = torch.empty(int(lib.ishara_op_scratch_bytes(M, K, N)) + 256, dtype=torch.uint8, device="cuda")
    scp = C.c_void_p(sc.data_ptr() + (-sc.data_ptr()) % 256)
    y = torch.full((M + 8, N), float("nan"), dtype=tdt, device="cuda")
    try:
        lib.ishara_debug_set_as_flags(flags)
        name = lib.ishara_debug_dense_kernel_name(1, M, K, N, 0, 0).decode()
        _lib.check(lib.ishara_op_dense_fwd_ex(code, _lib.ptr(xd), _lib.ptr(Wd), _lib.ptr(bd), None, _lib.ptr(y), M, K, N, 0, scp, stream()))
        torch.cuda.synchronize()
    finally:
        lib.ishara_debug_set_as_flags(-1)
    assert name == (NEW if flags == FORCED else TILE), (flags, name)
    assert bool(torch.isnan(y[M:].float()).all()), "rows behind M were written"
    return y[:M]


# 1 a single row | 200 partial first pass, no second | 256 first pass exactly | 257 second pass with one row | 384 one full workgroup |
# 1282 three full workgroups and a partial one
@pytest.mark.parametrize("M", [1, 200, 256, 257, 384, 1282])
def test_row_edges_against_fp64(lib, M):
    g = torch.Generator().manual_seed(17 * M + 5)
    x = torch.randn(M, K, generator=g).to(torch.bfloat16)
    W = torch.randn(K, N, generator=g) / K ** 0.5
    b = torch.randn(N, generator=g)
    y = _dense(lib, FORCED, x, W, b)
    ref = x.double() @ W.to(torch.bfloat16).double() + b.double()
    close(y, ref, "dense_c_stationary_k768", **TOL["bf16"])
    tile = _dense(lib, FORCED | OFF, x, W, b)
    print(f"M {M}: bit-identical to the tile kernel: {bool(torch.equal(y, tile))}")


def _ternary(M, seed):
    """A [M, K] and W [K, N] with entries in {-1, 0, 1}; W has at most 128 non-zeros per column: every output is an integer of magnitude <= 128,
    exact in fp32 accumulation in any order and in bf16 (checked here, on the host, for the seeds used)"""
    g = np.random.default_rng(seed)
    A = g.integers(-1, 2, size=(M, K)).astype(np.int64)
    W = np.zeros((K, N), np.int64)
    for n in range(N):
        nz = g.choice(K, size=int(g.integers(64, 129)), replace=False)
        W[nz, n] = g.choice(np.array([-1, 1]), size=nz.size)
    assert int((W != 0).sum(0).max()) <= 128 and int((W != 0).sum(0).min()) >= 64
    assert int(np.abs(A @ W).max()) <= 128
    return A, W


def _exact(lib, A, W, what):
    ref = A @ W
    assert int(np.abs(ref).max()) <= 128
    y = _dense(lib, FORCED, torch.from_numpy(A).to(torch.bfloat16), torch.from_numpy(W).float(), torch.zeros(N))
    got = y.float().cpu().numpy().astype(np.int64)
    assert np.array_equal(y.float().cpu().numpy(), got.astype(np.float32)), f"{what}: non-integer outputs"
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{what}: {len(bad)} elements differ from the int64 reference, first at {bad[0].tolist()}: {got[tuple(bad[0])]} != {ref[tuple(bad[0])]}"


@pytest.mark.parametrize("M", [384, 1282])
def test_exact_integer_case(lib, M):
    A, W = _ternary(M, 900 + M)
    _exact(lib, A, W, f"M {M}")


def test_one_case_per_k_chunk(lib):
    """A is non-zero only in one 32-k half of one 64-k chunk: the result is that half's product alone, exactly"""
    A, W = _ternary(384, 77)
    for s in range(12):
        for h in range(2):
            As = np.zeros_like(A)
            lo = 64 * s + 32 * h
            As[:, lo:lo + 32] = A[:, lo:lo + 32]
            assert np.abs(As @ W).max() > 0
            _exact(lib, As, W, f"chunk {s} half {h}")


def _route(lib, flags, M, **kw):
    """(route, kernel, last error) of ishara_debug_gemm_nt_route for a plain bf16 K = 768 -> N = 256 call with made-up aligned addresses.  The
    entry serves the tile kernels only: for another family it answers NT_REFUSED and names the route gemm_nt_route chose in its message."""
    k = _lib.GemmNtCall()
    v = dict(A=4096, Bt=8192, C=12288, dtA=1, dtM=1, dtC=1, M=M, N=N, K=K, bt_rows=256, ldb=K, tab_period=1, T=1, H=1, dh=1, head_major=1)
    v.update(kw)
    for n, x in v.items():
        setattr(k, n, x)
    route, kernel = C.c_char_p(), C.c_char_p()
    try:
        lib.ishara_debug_set_as_flags(flags)
        assert lib.ishara_debug_gemm_nt_route(C.byref(k), C.byref(route), C.byref(kernel)) == 0
        msg = (lib.ishara_last_error() or b"").decode() if route.value == b"NT_REFUSED" else ""
    finally:
        lib.ishara_debug_set_as_flags(-1)
    return route.value.decode(), kernel.value.decode(), msg


def _name(lib, flags, M, k=K, act=0, resid=0):
    try:
        lib.ishara_debug_set_as_flags(flags)
        return lib.ishara_debug_dense_kernel_name(1, M, k, N, act, resid).decode()
    finally:
        lib.ishara_debug_set_as_flags(-1)


def test_route_and_name(lib):
    for flags in (-1, 115):          # the library default and the same value stated
        assert _route(lib, flags, 49152)[:2] == ("NT_TILE_T", TILE)
        for M in (49153, 98304):
            route, kernel, msg = _route(lib, flags, M)
            assert (route, kernel) == ("NT_REFUSED", "") and "route NT_CS" in msg, (M, route, kernel, msg)
            assert _name(lib, flags, M) == NEW
            # a residual, an activation, a dact at K = 768 stay off the route
            assert _route(lib, flags, M, resid=20480)[:2] == ("NT_TILE_T", TILE)
            assert _route(lib, flags, M, act=1)[:2] == ("NT_TILE_T", TILE)
            assert _route(lib, flags, M, dact=1, aux=20480)[:2] == ("NT_TILE_T", TILE)
            assert "gemm_nt_cs" not in _name(lib, flags, M, resid=1) and "gemm_nt_cs" not in _name(lib, flags, M, act=1)
    for M in (49153, 98304):
        for flags in (115 | OFF, 51, 3):
            assert _route(lib, flags, M)[:2] == ("NT_TILE_T", TILE), (M, flags)
            assert _name(lib, flags, M) == TILE
        # the off bit is K = 768's alone, and the K = 512 names are what they were
        assert _name(lib, 115 | OFF, M, k=512) == "gemm_nt_cs_kernel<0,0>" == _name(lib, -1, M, k=512)
        assert _name(lib, 115, M, k=512, resid=1) == "gemm_nt_cs_kernel<1,0>"
    assert _name(lib, FORCED, 384) == NEW and _name(lib, FORCED | OFF, 384) == TILE
    assert "route NT_CS" in _route(lib, FORCED, 384)[2]


def test_mhsa_module_on_the_route():
    """cfg2, B = 2 (M = 768), bf16: the attention module with its QKV dgrad forced onto the new kernel, against the fp64 module reference at the
    bounds of tests/test_modules_gpu.py; the failure message says whether dx and the gradients equal the tile route's bit for bit."""
    name, dropout = "squeezeformer_0/mha", 0.2
    seen = []

    def routes(name_, kind, shape, dtype, dropout_, B, variant, report):
        seen.append(report)
        assert NEW in report, f"the forced route did not reach {NEW}: {report}"
        TM._check_routes(name_, kind, shape, dtype, dropout_, B, variant, report)

    lib = _lib.load()
    err = None
    try:
        lib.ishara_debug_set_as_flags(FORCED)
        TM.check_module("cfg2", "bf16", dropout, 2, "", name, log_test="gemm_cs_k768", check_routes=routes)
    except AssertionError as e:
        err = e
    finally:
        lib.ishara_debug_set_as_flags(-1)
    model, W, flat = TM._model("cfg2", "bf16", dropout, 2, "")
    y0, dx0, g0, rep0 = CS._run_module(model, flat, name, FORCED | OFF, True, dropout)
    y1, dx1, g1, rep1 = CS._run_module(model, flat, name, FORCED, True, dropout)
    same = {"y": bool(torch.equal(y0, y1)), "dx": bool(torch.equal(dx0, dx1)), **{n: bool(torch.equal(g0[n], g1[n])) for n in g0}}
    note = f"bit-identical to the tile route: {same}"
    print(note)
    assert NEW in rep1 and NEW not in rep0 and TILE in rep0, (rep0, rep1)
    assert seen, "the profiled route was not checked"
    if err is not None:
        raise AssertionError(f"{err}\n{note}")
