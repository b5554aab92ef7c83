"""The torch Squeezeformer family's own kernels (relattn_len.hip, r4_subsample.hip) against fp64, operator by operator, through the
ishara_op_relattn_* / ishara_op_r4_* entry points, which run the launch code of ishara_encoder_forward / _backward:

  relattn_len_fwd_kernel, relattn_len_bwd_dq / _dkv / _dpos without lengths (a NULL key_len: every key) and the two mixed-dtype pos_proj GEMMs
  (storage-dtype table, fp32 output / fp32 dy, M = 2T-1)
  r4_sub1_* / r4_sub2_* (DepthwiseConv2dSubsampling), r4_tred_fwd / _bwd_w / _bwd_x with the Linear over the padded K and its weight gradient
  through the [Kp, d] scratch and r4_axpy_f32, the five row maps r4_rows<MODE>.

The references, the cases and the bounds are tests/r4_parity.py's (fp64 on the operands the kernel receives; f32 at the operator bounds, bf16
at 2x observed; tests/test_r4_mutants.py shows that the bounds reject ordinary mistakes).  The attention's dropout mask is
oracle/rng.py's bit-exact restatement of the kernels' generator.  Observed errors are logged through test_model_gpu._log_observed."""
import ctypes as C

import numpy as np
import pytest
import torch

import r4_parity as R
from ishara_amd import _lib
from test_model_gpu import _log_observed

pytestmark = pytest.mark.gpu

DT = {"f32": (_lib.F32, torch.float32), "bf16": (_lib.BF16, torch.bfloat16)}


def dev(a, tdt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(tdt).cuda().contiguous()


def host(t):
    return t.float().cpu().numpy()


def _finish(test, case, dtype, obs, bad, **extra):
    _log_observed(dict(test=test, case=list(case), dtype=dtype, **extra, **obs))
    print(f"observed {obs}")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------ relative-position attention
def run_relattn(lib, case, dtype, seed, rate):
    B, H, T, dh = case
    d, Rr = H * dh, 2 * T - 1
    code, tdt = DT[dtype]
    inp = R.relattn_inputs(case, dtype)
    q, k, v, dO = (dev(inp[n], tdt) for n in ("q", "k", "v", "dO"))
    pe, Wpos, u, vb = (dev(inp[n]) for n in ("pe", "Wpos", "u", "vb"))
    o, dq, dk, dv = (torch.full((B * T, d), float("nan"), dtype=tdt, device="cuda") for _ in range(4))
    lse = torch.full((B * H * T,), float("nan"), device="cuda")
    du, dvb = (torch.full((d,), float("nan"), device="cuda") for _ in range(2))      # (the entry point overwrites every output)
    dWpos = torch.full((d, d), float("nan"), device="cuda")
    dposp = torch.full((Rr, d), float("nan"), device="cuda")
    nbytes = int(lib.ishara_op_relattn_scratch_bytes(B, H, T, dh))
    assert nbytes > 0
    keep, sc = _lib.aligned(nbytes, "cuda")
    P = _lib.ptr
    _lib.check(lib.ishara_op_relattn_fwd(code, P(q), P(k), P(v), P(pe), P(Wpos), P(u), P(vb), P(o), P(lse), B, H, T, dh, seed, R.SITE, C.c_float(rate), sc, _lib.stream()),
               "ishara_op_relattn_fwd")
    _lib.check(lib.ishara_op_relattn_bwd(code, P(q), P(k), P(v), P(u), P(vb), P(o), P(dO), P(dq), P(dk), P(dv), P(du), P(dvb), P(dWpos), P(dposp),
                                         B, H, T, dh, seed, R.SITE, C.c_float(rate), sc, _lib.stream()), "ishara_op_relattn_bwd")
    torch.cuda.synchronize()
    del keep
    r3 = lambda t: host(t).reshape(B, T, d)
    return dict(o=r3(o), lse=host(lse).reshape(B, H, T), dq=r3(dq), dk=r3(dk), dv=r3(dv), du=host(du), dvb=host(dvb), dposp=host(dposp), dWpos=host(dWpos))


_o_rate0 = {}


@pytest.mark.parametrize("rate", [0.0, R.RATE], ids=lambda r: f"drop{r}")
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.RELATTN_CASES, ids=lambda c: "B%d-H%d-T%d-dh%d" % c)
def test_relative_attention_matches_fp64(lib, case, dtype, rate):
    """o, lse, dq, dk, dv, du, dvb, dposp, dWpos of one attention call; with dropout the mask is the generator's, drawn by four kernels with three
    different index derivations"""
    B, H, T, dh = case
    seed = R.dropout_seed(case, rate) if rate > 0 else 4242
    got = run_relattn(lib, case, dtype, seed, rate)
    if rate == 0:
        _o_rate0[(case, dtype)] = got["o"]
    else:
        zeros = float((R.attn_mask(case, seed, rate) == 0).double().mean())
        assert 0.10 <= zeros <= 0.30, zeros
        base = _o_rate0.get((case, dtype))
        if base is None:
            base = run_relattn(lib, case, dtype, seed, 0.0)["o"]
        assert not np.array_equal(base, got["o"]), "the output with dropout equals the output without: no dropout was applied"
    ref = R.relattn_reference(case, dtype, seed, rate)
    obs, bad = R.compare(got, ref, R.bounds(dtype), B * T)
    _finish("r4_relattn", case, dtype, obs, bad, rate=rate)


# ------------------------------------------------------------------ DepthwiseConv2dSubsampling
@pytest.mark.parametrize("with_dx", [True, False], ids=["dx", "nodx"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.SUB_CASES, ids=lambda c: "B%d-T%d-F%d-d%d" % c)
def test_subsampling_matches_fp64(lib, case, dtype, with_dx):
    B, T0, Fin, d = case
    T1, F1, T2, F2 = R.sub_dims(T0, Fin)
    code, tdt = DT[dtype]
    inp = R.subsample_inputs(case, dtype)
    x, w1, b1, w2, b2 = (dev(inp[n]) for n in ("x", "w1", "b1", "w2", "b2"))
    dsub = dev(inp["dsub"], tdt)
    sub = torch.full((B * T2, d * F2), float("nan"), dtype=tdt, device="cuda")
    dw1, dw2 = (torch.full((d, 9), float("nan"), device="cuda") for _ in range(2))
    db1, db2 = (torch.full((d,), float("nan"), device="cuda") for _ in range(2))
    dx = torch.full((B, T0, Fin), float("nan"), device="cuda") if with_dx else None
    nbytes = int(lib.ishara_op_r4_subsample_scratch_bytes(B, T0, Fin, d))
    assert nbytes > 0
    keep, sc = _lib.aligned(nbytes, "cuda")
    P = _lib.ptr
    _lib.check(lib.ishara_op_r4_subsample_fwd(code, P(x), P(w1), P(b1), P(w2), P(b2), P(sub), B, T0, Fin, d, sc, _lib.stream()), "ishara_op_r4_subsample_fwd")
    _lib.check(lib.ishara_op_r4_subsample_bwd(code, P(x), P(w1), P(w2), P(sub), P(dsub), P(dw1), P(db1), P(dw2), P(db2), P(dx), B, T0, Fin, d, sc, _lib.stream()),
               "ishara_op_r4_subsample_bwd")
    torch.cuda.synchronize()
    got = dict(sub=host(sub), dw1=host(dw1), db1=host(db1), dw2=host(dw2), db2=host(db2))
    names = ["sub", "dw1", "db1", "dw2", "db2"]
    if with_dx:
        got["dx"] = host(dx)
        names.append("dx")
    ref = R.subsample_reference(case, dtype)
    obs, bad = R.compare(got, ref, R.bounds(dtype), B * T2 * F2, ref["alts"], names)
    _finish("r4_subsample", case, dtype, obs, bad, with_dx=with_dx)


# ------------------------------------------------------------------ TimeReductionLayer + time_reduction_proj
@pytest.mark.parametrize("with_extra", [True, False], ids=["extra", "noextra"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", R.TRED_CASES, ids=lambda c: "B%d-T%d-d%d" % c)
def test_time_reduction_matches_fp64(lib, case, dtype, with_extra):
    B, Tin, d = case
    Tr, Fr, Kp = R.tred_dims(Tin, d)
    code, tdt = DT[dtype]
    inp = R.tred_inputs(case, dtype)
    h, dred = dev(inp["h"], tdt), dev(inp["dred"], tdt)
    extra = dev(inp["extra"], tdt) if with_extra else None
    cw, cb, Wred, bred = (dev(inp[n]) for n in ("conv_w", "conv_b", "Wred", "bred"))
    red = torch.full((B * Tr, d), float("nan"), dtype=tdt, device="cuda")
    conv = torch.full((B * Tr, Kp), float("nan"), dtype=tdt, device="cuda")
    dh = torch.full((B, Tin, d), float("nan"), dtype=tdt, device="cuda")
    dcw, dcb = torch.full((12,), float("nan"), device="cuda"), torch.full((4,), float("nan"), device="cuda")
    dWred, dbred = torch.full((Fr, d), float("nan"), device="cuda"), torch.full((d,), float("nan"), device="cuda")
    nbytes = int(lib.ishara_op_r4_time_reduce_scratch_bytes(B, Tin, d))
    assert nbytes > 0
    keep, sc = _lib.aligned(nbytes, "cuda")
    P = _lib.ptr
    _lib.check(lib.ishara_op_r4_time_reduce_fwd(code, P(h), P(cw), P(cb), P(Wred), P(bred), P(red), P(conv), B, Tin, d, sc, _lib.stream()), "ishara_op_r4_time_reduce_fwd")
    _lib.check(lib.ishara_op_r4_time_reduce_bwd(code, P(h), P(cw), P(dred), P(extra), P(dh), P(dcw), P(dcb), P(dWred), P(dbred), B, Tin, d, sc, _lib.stream()),
               "ishara_op_r4_time_reduce_bwd")
    torch.cuda.synchronize()
    got = dict(red=host(red), dh=host(dh), dconv_w=host(dcw)[:9], dconv_b=host(dcb)[:1], dWred=host(dWred), dbred=host(dbred))
    assert np.isnan(host(dcw)[9:]).all() and np.isnan(host(dcb)[1:]).all(), "the conv gradients were written past their 9 / 1 elements"
    # the pad columns of the conv output (the Linear's zero-padded K) are exactly 0
    assert np.array_equal(host(conv)[:, Fr:], np.zeros((B * Tr, Kp - Fr), np.float32)), "pad columns of the conv output are not zero"
    # dh rows / columns that no output reads (t > 2 Tr, f > 2 Fr) are extra (or 0) exactly
    want = inp["extra"] if with_extra else np.zeros((B, Tin, d), np.float32)
    assert np.array_equal(got["dh"][:, 2 * Tr + 1:], want[:, 2 * Tr + 1:]), "dh rows no output reads differ from extra"
    assert np.array_equal(got["dh"][:, :, 2 * Fr + 1:], want[:, :, 2 * Fr + 1:]), "dh columns no output reads differ from extra"
    ref = R.tred_reference(case, dtype, with_extra)
    obs, bad = R.compare(got, ref, R.bounds(dtype), B * Tr)
    _finish("r4_time_reduce", case, dtype, obs, bad, with_extra=with_extra)


# ------------------------------------------------------------------ row maps
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B,T2,T3,d", [(3, 37, 18, 24), (2, 8, 3, 16)])
def test_row_maps_are_exact(lib, B, T2, T3, d, dtype):
    """modes 0, 1, 3 copy (array-equal to torch indexing); modes 2, 4 add two storage-dtype values in fp32 and round once"""
    code, tdt = DT[dtype]
    Trec = 2 * T3
    g = torch.Generator().manual_seed(B * 1000 + T2)
    draw = lambda T: torch.randn(B, T, d, generator=g).to(tdt).cuda()
    short, long_, rec, rec2 = draw(T3), draw(T2), draw(Trec), draw(Trec)

    def rows(mode, src, a, Tdst, Tsrc):
        dst = torch.full((B, Tdst, d), float("nan"), dtype=tdt, device="cuda")
        _lib.check(lib.ishara_op_r4_rows(code, mode, _lib.ptr(src), _lib.ptr(a), _lib.ptr(dst), B, Tdst, Tsrc, d, _lib.stream()), f"ishara_op_r4_rows mode {mode}")
        torch.cuda.synchronize()
        return dst

    assert torch.equal(rows(0, short, None, Trec, T3), torch.repeat_interleave(short, 2, dim=1))                      # recover_resolution
    assert torch.equal(rows(1, long_, None, Trec, T2), long_[:, :Trec])                                              # crop of the longer sequence
    want3 = torch.zeros(B, T2, d, dtype=tdt, device="cuda")
    want3[:, :Trec] = rec
    assert torch.equal(rows(3, rec, None, T2, Trec), want3)                                                          # backward of the crop
    assert torch.equal(rows(2, rec, None, T3, Trec), (rec[:, 0::2].float() + rec[:, 1::2].float()).to(tdt))          # backward of recover_resolution
    assert torch.equal(rows(4, rec, rec2, Trec, Trec), (rec.float() + rec2.float()).to(tdt))                         # the wrapper's residual
