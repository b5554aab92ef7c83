"""The depthwise-conv backward kernels against fp64 through ishara_op_dwconv_bwd, ishara_op_dwconv_bwd_bn and ishara_op_bn_bwd_apply, at the
segment, tile, lane and item-loop edges of each: the cases, the reference, the counting inputs and the bounds are tests/dwconv_parity.py's
(tests/test_dwconv_mutants.py shows that they reject ordinary mistakes).  Every case asserts first that the route picks the kernel the case is
for.  dx, dw, dbias, the scratch and tmp lie between 4 KiB guards; dx starts as NaN bytes, dw and dbias at 0.25 and -0.5 (they are accumulated
into), the scratch as 0xFF bytes in one run and as zeros in another, between which every output must agree bit for bit (dw / dbias of the atomic
weight gradient excepted).  Observed figures are printed and appended to the file ISHARA_DW_LOG names."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import dwconv_parity as D
from ishara_amd import _lib

pytestmark = pytest.mark.gpu

DT = {"f32": (_lib.F32, torch.float32), "bf16": (_lib.BF16, torch.bfloat16)}
GUARD = 4096
GUARD_BYTE, NAN_BYTE = 0xA5, 0xFF      # 0xFFFF is a bf16 NaN, 0xFFFFFFFF an fp32 NaN


class Guarded:
    """`nbytes` of `fill` bytes at a 256-byte aligned device address between two 4 KiB guard regions"""

    def __init__(self, nbytes, fill=NAN_BYTE):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD + 256,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.off = (-self.buf.data_ptr()) % 256 + GUARD
        self.buf[self.off:self.off + self.n] = fill
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.off)

    def view(self, tdt):
        return self.buf[self.off:self.off + self.n].view(tdt)

    def guards_intact(self):
        return bool((self.buf[:self.off] == GUARD_BYTE).all() and (self.buf[self.off + self.n:] == GUARD_BYTE).all())


def _dev(a, tdt=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(tdt).cuda().contiguous()


def run(lib, c, op, scratch_fill=NAN_BYTE, inop=None, two_launch=False):
    """one backward call on the operands `op` -> (dx, dw, dbias or None as device tensors, what the entry point answered).  With a BatchNorm
    the call is ishara_op_dwconv_bwd_bn, or (two_launch) ishara_op_bn_bwd_apply into tmp followed by ishara_op_dwconv_bwd on tmp."""
    inop = c.inop if inop is None else inop
    code, tdt = DT[c.dtype]
    es = 2 if c.dtype == "bf16" else 4
    B, T, Cc, k = c.B, c.T, c.C, c.k
    Cin = op["x"].shape[-1]
    x, dy, w = _dev(op["x"], tdt), _dev(op["dy"], tdt), _dev(op["w"])
    dx, dw, dbias = Guarded(B * T * Cin * es), Guarded(k * Cc * 4), Guarded(Cc * 4) if c.bias else None
    dw.view(torch.float32)[:] = D.DW_START
    if dbias is not None:
        dbias.view(torch.float32)[:] = D.DBIAS_START
    scr = Guarded(int(lib.ishara_op_dwconv_scratch_bytes(Cc, k)), scratch_fill) if c.scratch else None
    tmp = Guarded(B * T * Cc * es) if c.bn else None
    shape = (B, T, Cc, k, c.padl, _lib.stream())
    outs = (dx.ptr, dw.ptr, dbias.ptr if dbias is not None else None, scr.ptr if scr is not None else None)
    rc = 0
    lib.ishara_debug_force_regstage(D.FORCE_LDS if c.force else 0)
    try:
        if not c.bn:
            _lib.check(lib.ishara_op_dwconv_bwd(code, inop, _lib.ptr(dy), _lib.ptr(x), _lib.ptr(w), *outs, *shape), "ishara_op_dwconv_bwd")
        else:
            h = _dev(op["h"], tdt)
            mean, rstd, a, sg, E, Fc = (_dev(op[n]) for n in ("mean", "rstd", "a", "sg", "E", "Fc"))
            bn = (_lib.ptr(h), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(a), _lib.ptr(sg), _lib.ptr(E), 1 if op["E"].ndim == 2 else 0, _lib.ptr(Fc))
            if two_launch:
                _lib.check(lib.ishara_op_bn_bwd_apply(code, _lib.ptr(dy), *bn, tmp.ptr, B, T, Cc, _lib.stream()), "ishara_op_bn_bwd_apply")
                _lib.check(lib.ishara_op_dwconv_bwd(code, inop, tmp.ptr, _lib.ptr(x), _lib.ptr(w), *outs, *shape), "ishara_op_dwconv_bwd")
            else:
                rc = lib.ishara_op_dwconv_bwd_bn(code, inop, _lib.ptr(dy), *bn, _lib.ptr(x), _lib.ptr(w), *outs, tmp.ptr, *shape)
                if rc < 0:
                    _lib.check(rc, "ishara_op_dwconv_bwd_bn")
        torch.cuda.synchronize()
    finally:
        lib.ishara_debug_force_regstage(0)
    for name, gb in (("dx", dx), ("dw", dw), ("dbias", dbias), ("scratch", scr), ("tmp", tmp)):
        assert gb is None or gb.guards_intact(), f"a guard region of {name} was written"
    if c.bn and not two_launch and rc == 1:
        assert bool((tmp.view(torch.uint8) == NAN_BYTE).all()), "the one-pass kernel ran and tmp was written"
    return dict(dx=dx.view(tdt).clone(), dw=dw.view(torch.float32).clone(), dbias=dbias.view(torch.float32).clone() if dbias is not None else None), rc


def host(c, out, Cin):
    """fp64 arrays, dw / dbias without their start values"""
    got = dict(dx=out["dx"].double().cpu().numpy().reshape(c.B, c.T, Cin), dw=out["dw"].double().cpu().numpy().reshape(c.k, c.C) - D.DW_START)
    if out["dbias"] is not None:
        got["dbias"] = out["dbias"].double().cpu().numpy() - D.DBIAS_START
    return got


def bit_equal(a, b, names):
    return [n for n in names if a[n] is not None and not torch.equal(a[n].view(torch.uint8), b[n].view(torch.uint8))]


def ulp_of(m, dtype):
    """one unit in the last place of the storage dtype at magnitude m"""
    return 2.0 ** (np.floor(np.log2(np.maximum(m, 1e-37))) - (7 if dtype == "bf16" else 23))


def _log(c, **fields):
    print(D.case_id(c), c.kernel, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in fields.items()})
    path = os.environ.get("ISHARA_DW_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=D.case_id(c), **c._asdict(), **fields)) + "\n")


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_dwconv_backward_matches_fp64(lib, c):
    assert D.expected_kernel(lib, c) == c.kernel, "the route does not pick the kernel this case is for"
    op = D.inputs(c)
    Cin = op["x"].shape[-1]
    names = ("dx", "dw", "dbias")
    out, rc = run(lib, c, op, scratch_fill=0xFF)
    out0, rc0 = run(lib, c, op, scratch_fill=0x00)
    if c.bn:
        assert rc == rc0 == (1 if c.kernel == D.FUSED_BN else 0), "ishara_op_dwconv_bwd_bn: folded where the route has no such kernel, or the reverse"
    # the partial rows need no initialisation, and (with a scratch) the row sums have a fixed order: bit for bit, run to run
    differ = bit_equal(out, out0, ("dx",) if D.is_atomic(c) else names)
    assert not differ, f"{differ} depend on what the scratch held, or differ run to run"
    obs = D.observe(c, host(c, out, Cin), D.reference(c, op))
    extra = {}
    if c.bn and rc == 1:
        two, _ = run(lib, c, op, two_launch=True)
        a, b = out["dx"].double().cpu().numpy(), two["dx"].double().cpu().numpy()
        extra["dx_differ"] = int((a != b).sum())
        extra["dx_differ_ulp"] = float((np.abs(a - b) / ulp_of(np.maximum(np.abs(a), np.abs(b)), c.dtype)).max())
        extra["dw_differ"] = int((out["dw"] != two["dw"]).sum())
    _log(c, **obs, **extra)
    assert not D.excess(obs, D.bounds(c)), D.excess(obs, D.bounds(c))
    if "dx_differ_ulp" in extra:
        assert extra["dx_differ_ulp"] <= 1.0, f"one-pass and two-launch dx differ by {extra['dx_differ_ulp']} storage ulp in {extra['dx_differ']} elements"


@pytest.mark.parametrize("c", D.CASES, ids=D.case_id)
def test_dwconv_backward_counts_every_row_once(lib, c):
    """dy = 1, x = 1: dbias = B T, dw = B x the steps each tap meets, dx = the taps in range — integers (quarters), so equality"""
    op = D.counting_inputs(c)
    out, _ = run(lib, c, op, inop=D.NONE)
    got, want = host(c, out, c.C), D.counting_expect(c, op["w"])
    for n in ("dbias", "dw", "dx"):
        if n in got:
            bad = np.argwhere(got[n] != want[n])
            assert not len(bad), f"{n}: {len(bad)} elements differ, first at {tuple(bad[0])}: got {got[n][tuple(bad[0])]}, exact {want[n][tuple(bad[0])]}"
