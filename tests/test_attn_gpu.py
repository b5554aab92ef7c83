"""The training attention kernels (attention.hip's lane-split kernels, attention_mfma.hip's MFMA forward, attention_bwd_mfma.hip's one-pass backward in all eight
(waves, tiles, FULL / ragged) forms and its two-kernel backward at dh 32 and 64) against fp64 through ishara_op_attn_fwd / _bwd, at the tile
edges of each: the cases, the reference and the bounds are tests/attn_parity.py's (f32 at the operator bound, bf16 at 2x observed once
measured; tests/test_attn_mutants.py shows that the bounds reject ordinary mistakes).  Compared: o, lse, dq, dk, dv and, on the routes that store it,
delta (against rowsum(dO o o) of the kernel's own o).  o, dqkv and the scratch lie between 4 KiB guards, o, dqkv and the whole scratch start as
NaN bytes, and the padding between lse, delta and the keep-bit words (ishara_op_attn_scratch_layout_bytes) must come back untouched.  Observed
figures are printed and appended to the file ISHARA_ATTN_LOG names."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import attn_parity as A
from ishara_amd import _lib

pytestmark = pytest.mark.gpu

DT = {"f32": (_lib.F32, torch.float32), "bf16": (_lib.BF16, torch.bfloat16)}
GUARD = 4096
GUARD_BYTE, NAN_BYTE = 0xA5, 0xFF      # 0xFFFF is a bf16 NaN, 0xFFFFFFFF an fp32 NaN
TWO_PASS = A.TWO_PASS


class Guarded:
    """`nbytes` of NaN bytes at a 256-byte aligned device address between two 4 KiB guard regions"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD + 256,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.off = (-self.buf.data_ptr()) % 256 + GUARD
        self.buf[self.off:self.off + self.n] = NAN_BYTE
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.off)

    def payload(self):
        return self.buf[self.off:self.off + self.n]

    def view(self, tdt, count, byte_off=0):
        return self.payload()[byte_off:byte_off + count * torch.empty((), dtype=tdt).element_size()].view(tdt)

    def guards_intact(self):
        return bool((self.buf[:self.off] == GUARD_BYTE).all() and (self.buf[self.off + self.n:] == GUARD_BYTE).all())


def layout(lib, shp):
    out = (C.c_int64 * 6)()
    _lib.check(lib.ishara_op_attn_scratch_layout_bytes(*shp, out), "ishara_op_attn_scratch_layout_bytes")
    return dict(zip(("lse", "delta", "maskw"), ((int(out[2 * i]), int(out[2 * i + 1])) for i in range(3))))


def run(lib, c):
    """one forward and one backward call -> (tensors as attn_parity.reference returns them, raw o / dqkv for bit comparisons)"""
    B, H, T, dh = shp = A.shape(c)
    d = H * dh
    code, tdt = DT[c.dtype]
    es = 2 if c.dtype == "bf16" else 4
    qkv, dO = A.inputs(c)
    qd, dd = (torch.from_numpy(a).to(tdt).cuda().contiguous() for a in (qkv, dO))
    total = int(lib.ishara_op_attn_scratch_bytes(*shp))
    lay = layout(lib, shp)
    o, dqkv, sc = Guarded(B * T * d * es), Guarded(B * T * 3 * d * es), Guarded(total)
    seed, f = A.seed_of(c), C.c_float
    args = (B, H, T, dh, f(A.scale_of(c)), seed, A.SITE, f(c.rate), A.impl(c), sc.ptr, _lib.stream())
    assert A.bwd_kernel(lib, c), "the route refuses the backward call"
    lib.ishara_debug_force_regstage(TWO_PASS if c.two_pass else 0)
    try:
        _lib.check(lib.ishara_op_attn_fwd(code, _lib.ptr(qd), o.ptr, *args), "ishara_op_attn_fwd")
        _lib.check(lib.ishara_op_attn_bwd(code, o.ptr, _lib.ptr(dd), dqkv.ptr, *args), "ishara_op_attn_bwd")
        torch.cuda.synchronize()
    finally:
        lib.ishara_debug_force_regstage(0)
    for name, gb in (("o", o), ("dqkv", dqkv), ("scratch", sc)):
        assert gb.guards_intact(), f"a guard region of {name} was written"
    # the padding inside the scratch: from each region's extent to the next region's offset (the end of the scratch for the keep-bit words)
    ends = [lay["delta"][0], lay["maskw"][0], total]
    for (name, (off, ext)), end in zip(lay.items(), ends):
        assert off % 256 == 0 and off + ext <= end, (name, off, ext, end)
        assert bool((sc.payload()[off + ext:end] == NAN_BYTE).all()), f"the padding after {name} ({end - off - ext} bytes) was written"
    host = lambda t: t.float().cpu().numpy()
    o_t, dqkv_t = o.view(tdt, B * T * d), dqkv.view(tdt, B * T * 3 * d)
    dq, dk, dv = A.split(host(dqkv_t), shp)
    got = dict(o=host(o_t).reshape(B, T, d), lse=host(sc.view(torch.float32, B * H * T, lay["lse"][0])).reshape(B, H, T), dq=dq, dk=dk, dv=dv)
    if A.writes_delta(lib, c):
        got["delta"] = host(sc.view(torch.float32, B * H * T, lay["delta"][0])).reshape(B, H, T)
    return got, dict(o=o_t.clone(), dqkv=dqkv_t.clone())


def _log(lib, c, obs, **extra):
    kernel = A.bwd_kernel(lib, c)
    print(A.case_id(c), kernel, {k: f"{v:.3g}" for k, v in obs.items()}, extra or "")
    path = os.environ.get("ISHARA_ATTN_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=A.case_id(c), kernel=kernel, **c._asdict(), **obs, **extra)) + "\n")


_raw = {}      # case -> raw o / dqkv of the cases other cases are compared with bit by bit


def _raw_of(lib, c):
    if c not in _raw:
        _raw[c] = run(lib, c)[1]
    return _raw[c]


@pytest.mark.parametrize("c", A.CASES, ids=A.case_id)
def test_attention_matches_fp64(lib, c):
    got, raw = run(lib, c)
    _raw[c] = raw
    ref = dict(A.reference(c))
    names = ["o", "lse", "dq", "dk", "dv"]
    if A.writes_delta(lib, c):
        assert np.isfinite(got["o"]).all(), "o is not finite"
        ref["delta"] = A.delta_from(got["o"], A.inputs(c)[1], A.shape(c))      # delta is defined on the kernel's own (rounded) o
        names.append("delta")
    obs, bad = A.compare(got, ref, A.bounds(c), names)
    extra = {}
    if c.rate > 0:
        mask = A.mask_of(A.shape(c), A.seed_of(c), c.rate)
        if mask is not None and mask.numel() >= 4096:
            lo, hi = A.mask_share_range(c.rate)
            extra["mask_zero_share"] = share = float((mask == 0).double().mean())
            assert lo <= share <= hi, share
            base = _raw_of(lib, c._replace(rate=0.0, dm=0))["o"]
            assert not torch.equal(base, raw["o"]), "the output with dropout equals the output without: no dropout was applied"
        if c.dm == 1:      # the same mask hashed again in the backward kernels instead of read back: how far the two routes differ
            other = _raw_of(lib, c._replace(dm=2))
            extra["o_differs_from_dm2"] = int((other["o"] != raw["o"]).sum())
            extra["dqkv_differs_from_dm2"] = int((other["dqkv"] != raw["dqkv"]).sum())
    if c.regime == "q0":      # a uniform softmax in closed form: lse = log T, o = the mean of v over the keys
        B, H, T, dh = A.shape(c)
        assert np.abs(got["lse"] - np.log(T)).max() <= 2e-5, "lse of a uniform softmax is not log T"
        vbar = A.inputs(c)[0].astype(np.float64).reshape(B, T, H, 3 * dh)[..., 2 * dh:].mean(1)      # [B, H, dh]
        err = np.abs(got["o"].reshape(B, T, H, dh) - vbar[:, None])
        # every P is exp(0) = 1, exact in bf16: what is left is the fp32 sum (2e-5, as for lse) and, in bf16, o's own rounding: half an ulp is
        # 2^-9 |o|, allowed twice
        assert bool((err <= 2e-5 + (2.0 ** -8 if c.dtype == "bf16" else 0.0) * np.abs(vbar[:, None])).all()), "o of a uniform softmax is not the mean of v"
    _log(lib, c, obs, **extra)
    assert not bad, "\n".join(bad)


def test_a_rate_that_rounds_to_no_dropout_changes_nothing(lib):
    """rate 0.001: thr8 = round(0.256) = 0, every key is kept and the scale is 1: o and dqkv are bit-equal to the rate-0 run"""
    c = A.TINY_RATE_CASE
    a, b = run(lib, c)[1], _raw_of(lib, c._replace(rate=0.0, dm=0))
    assert torch.equal(a["o"], b["o"]) and torch.equal(a["dqkv"], b["dqkv"])
