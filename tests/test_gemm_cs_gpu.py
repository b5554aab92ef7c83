"""The C-stationary GEMM of the K = 512 -> N = 256 projections (gemm_cs.hip, gemm_nt_cs_kernel<MASK,PRO>) against the A-stationary kernels it
replaces at training-size M.  Same MFMA instruction, operand order, ascending order over K and epilogue arithmetic, so every output is
BIT-IDENTICAL to the per-step A-stationary kernel (as_flags 3); as_flags bits 64 | 128 force the new route at the small row counts used here:
the edges of its 256 + 128 row split, and B = 2 modules for the dropout / row-scale / per-sample-affine instantiations."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import module_parity as MP
import test_modules_gpu as TM
from ishara_amd import _lib
from test_ops_gpu import DT, TOL, close, dev, stream

pytestmark = pytest.mark.gpu

OLD, FORCED = 3, 3 | 64 | 128
K, N = 512, 256
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _operands(M, with_resid, n=N):
    code, tdt = DT["bf16"]
    g = torch.Generator().manual_seed(11 * M + n + int(with_resid))
    x = torch.randn(M, K, generator=g).to(tdt)
    W = torch.randn(K, n, generator=g) / K ** 0.5
    b = torch.randn(n, generator=g)
    r = torch.randn(M, n, generator=g).to(tdt) if with_resid else None
    return x, W, b, r


def _dense(lib, flags, x, W, b, r, act=0):
    code, tdt = DT["bf16"]
    M, n = x.shape[0], W.shape[1]
    xd, Wd, bd = x.cuda().contiguous(), dev(W), dev(b)
    rd = r.cuda().contiguous() if r is not None else None
    sc = torch.empty(int(lib.ishara_op_scratch_bytes(M, K, n)) + 256, dtype=torch.uint8, device="cuda")
    scp = C.c_void_p(sc.data_ptr() + (-sc.data_ptr()) % 256)
    y = torch.full((M + 8, n), float("nan"), dtype=tdt, device="cuda")       # 8 guard rows behind the output
    try:
        lib.ishara_debug_set_as_flags(flags)
        _lib.check(lib.ishara_op_dense_fwd_ex(code, _lib.ptr(xd), _lib.ptr(Wd), _lib.ptr(bd), _lib.ptr(rd), _lib.ptr(y), M, K, n, act, scp, stream()))
        torch.cuda.synchronize()
    finally:
        lib.ishara_debug_set_as_flags(-1)
    assert bool(torch.isnan(y[M:].float()).all()), "rows behind M were written"
    return y[:M]


def _ref(x, W, b, r, act=0):
    ref = x.double() @ W.to(torch.bfloat16).double() + b.double()
    ref = [ref, ref * torch.sigmoid(ref)][act]
    return ref + r.double() if r is not None else ref


# 1 a single row | 200 partial first pass, no second | 256 first pass exactly | 257 second pass with one row | 384 one full workgroup |
# 1282 three full workgroups and a partial one
@pytest.mark.parametrize("with_resid", [False, True])
@pytest.mark.parametrize("M", [1, 200, 256, 257, 384, 1282])
def test_dense_c_stationary_matches_a_stationary(lib, M, with_resid):
    x, W, b, r = _operands(M, with_resid)
    old = _dense(lib, OLD, x, W, b, r)
    new = _dense(lib, FORCED, x, W, b, r)
    assert torch.equal(old, new), f"C-stationary vs A-stationary: {int((old != new).sum())} elements differ, max {(old.float() - new.float()).abs().max().item()}"
    close(new, _ref(x, W, b, r), "dense_c_stationary", **TOL["bf16"])


def test_route_refuses_other_masks(lib):
    """an activation is not one of the kernel's masks: the forced flags fall through to the A-stationary kernel"""
    x, W, b, r = _operands(640, False)
    old = _dense(lib, OLD, x, W, b, r, act=1)
    new = _dense(lib, FORCED, x, W, b, r, act=1)
    assert torch.equal(old, new)
    close(new, _ref(x, W, b, r, act=1), "dense_swish", **TOL["bf16"])


def test_c_stationary_run_to_run(lib):
    x, W, b, r = _operands(1282, True)
    a = _dense(lib, FORCED, x, W, b, r)
    c = _dense(lib, FORCED, x, W, b, r)
    assert torch.equal(a, c), f"two runs differ in {int((a != c).sum())} elements"


def _kernel(lib, flags, M, with_resid, act=0, n=N):
    try:
        lib.ishara_debug_set_as_flags(flags)
        return lib.ishara_debug_dense_kernel_name(1, M, K, n, act, int(with_resid)).decode()
    finally:
        lib.ishara_debug_set_as_flags(-1)


ON = 115          # = the library default: the A-stationary kernels' 51 | 64, the route on, with its row threshold


def test_default_route_and_row_threshold(lib):
    """The two routes give identical outputs, so WHICH kernel a call takes is read from the route itself (ishara_debug_dense_kernel_name: the
    profiler key of the kernel the same dense call would launch).  The library default (-1) is as_flags 115, the route on; 51 and 3 never take it.
    With it on: M = 768 and M = 49152 (where the A-stationary launcher still splits the columns) stay on the A-stationary
    kernels, M = 49153 and the benchmark's 98304 take the C-stationary one; bit 128 drops the threshold; masks and shapes that are not the
    kernel's fall through."""
    x, W, b, r = _operands(768, True)
    assert torch.equal(_dense(lib, -1, x, W, b, r), _dense(lib, OLD, x, W, b, r))
    for resid, key in ((False, "gemm_nt_cs_kernel<0,0>"), (True, "gemm_nt_cs_kernel<1,0>")):
        for M in (768, 32768, 49152):
            assert _kernel(lib, ON, M, resid).startswith("gemm_nt_as_"), (M, _kernel(lib, ON, M, resid))
        for M in (768, 49152, 49153, 98304):
            assert _kernel(lib, -1, M, resid) == _kernel(lib, ON, M, resid), (M, _kernel(lib, -1, M, resid))
            assert "gemm_nt_cs" not in _kernel(lib, 51, M, resid) and "gemm_nt_cs" not in _kernel(lib, OLD, M, resid)
        for M in (49153, 98304):
            assert _kernel(lib, ON, M, resid) == key, (M, _kernel(lib, ON, M, resid))
            assert _kernel(lib, 51, M, resid).startswith("gemm_nt_as_chunk_kernel<bf16,16,"), _kernel(lib, 51, M, resid)
            assert _kernel(lib, OLD, M, resid).startswith("gemm_nt_as_kernel<bf16,16,")
            assert "gemm_nt_cs" not in _kernel(lib, ON, M, resid, act=1)           # a mask the kernel does not have
            assert "gemm_nt_cs" not in _kernel(lib, ON, M, resid, n=512)           # another N
        assert _kernel(lib, FORCED, 768, resid) == key
        assert "gemm_nt_cs" not in _kernel(lib, FORCED, 768, resid, act=1)
    for doc in ("INTEGRATION.md", os.path.join("include", "ishara_hip.h")):
        assert "ISHARA_AS_FLAGS" in open(os.path.join(ROOT, doc)).read(), f"ISHARA_AS_FLAGS is not documented in {doc}"


CS_KEYS = ["gemm_nt_cs_kernel<0,0>", "gemm_nt_cs_kernel<1,0>", "gemm_nt_cs_kernel<9,0>", "gemm_nt_cs_kernel<1,2>", "gemm_nt_cs_kernel<17,2>"]
MODULES = ["convsqueeze_0_1", "squeezeformer_0/ffn1", "conformer_0/ffn1", "squeezeformer_0/conv"]


def _run_module(model, flat, name, flags, profiled, dropout=0.2):
    lib = model._lib
    names = model.module_names()
    i = names.index(name)
    _, cin, cout, first, nsites = model._module_info(i)
    B, T = 2, 384
    g = np.random.default_rng(1000 + i)
    x = MP.round_to(g.standard_normal((B, T, cin)), "bf16")
    dy = MP.round_to(g.standard_normal((B, T, cout)), "bf16")
    seed = 4242
    if MP.module_kind(name) == "conv" and dropout > 0:
        seed = MP.mixed_droppath_seed(seed, first, B, dropout)
    model.params.copy_(flat)
    report = None
    try:
        lib.ishara_debug_set_as_flags(flags)
        if profiled:
            _lib.check(lib.ishara_profile_enable(model._h, 1))
        try:
            y = model.module_forward(i, x, training=True, seed=seed)
            dx = model.module_backward(i, dy)
            torch.cuda.synchronize()
            if profiled:
                report = TM._report(model)
        finally:
            if profiled:
                lib.ishara_profile_enable(model._h, 0)
    finally:
        lib.ishara_debug_set_as_flags(-1)
        model.params.copy_(flat)
    _lib.check(lib.ishara_workspace_guard_check(model._h), "workspace guard (a kernel wrote outside its buffer)")
    gflat = model.grads[:model.n_train].clone()
    grads = {n: gflat[o:o + int(np.prod(s))] for n, s, o, t in model.entries if t and MP.owns(name, n)}
    return y.clone(), dx.clone(), grads, report


def test_modules_bit_identical_on_the_c_stationary_route():
    """cfg2, B = 2 (M = 768), bf16, dropout 0.2: the four modules whose K = 512 -> N = 256 GEMMs carry dropout, the drop-path row scale and the
    per-sample-affine prologue.  y, dx and every parameter gradient are bit-identical between the two routes, as the product runs the module and
    under the profiler; the profiled reports name all five instantiations on the forced route and none on the old one.  With dropout on, a
    Conv1DBlock's project GEMM always carries the drop-path row scale (<17,2>); the prologue instantiation without it (<1,2>) is what the same
    block runs at dropout 0, so convsqueeze_0_1 runs once more on such a model."""
    seen = set()
    for dropout, modules in ((0.2, MODULES), (0.0, MODULES[:1])):
        model, W, flat = TM._model("cfg2", "bf16", dropout, 2, "")
        for name in modules:
            for profiled in (False, True):
                y0, dx0, g0, rep0 = _run_module(model, flat, name, OLD, profiled, dropout)
                y1, dx1, g1, rep1 = _run_module(model, flat, name, FORCED, profiled, dropout)
                assert torch.equal(y0, y1), f"{name} dropout {dropout}: y differs in {int((y0 != y1).sum())} elements"
                assert torch.equal(dx0, dx1), f"{name} dropout {dropout}: dx differs in {int((dx0 != dx1).sum())} elements"
                assert g0.keys() == g1.keys() and g0
                for n in g0:
                    assert torch.equal(g0[n], g1[n]), f"{name} dropout {dropout}: gradient of {n} differs"
                if profiled:
                    assert not any(k.startswith("gemm_nt_cs_kernel") for k in rep0), f"{name}: as_flags 3 reached the C-stationary kernel: {rep0}"
                    new = {k for k in rep1 if k.startswith("gemm_nt_cs_kernel")}
                    assert new, f"{name} dropout {dropout}: the forced route reached no C-stationary kernel: {rep1}"
                    assert dropout > 0 or "gemm_nt_cs_kernel<1,2>" in new, f"{name} dropout 0: {sorted(new)}"
                    seen |= new
    assert seen == set(CS_KEYS), f"instantiations reached: {sorted(seen)}, expected {CS_KEYS}"
