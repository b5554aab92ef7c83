"""Helpers of tests/test_ops_r4_gpu.py and tests/test_r4_mutants.py: the cases, the inputs and the fp64 references of the torch Squeezeformer
family's own operators (relative-position attention, DepthwiseConv2dSubsampling, TimeReductionLayer + time_reduction_proj), with switchable
mistakes, and the bounds.  The references are the functions of oracle/squeezeformer_torch_oracle.py (pinned to the reference's own files by
tests/test_golden_squeezeformer.py) evaluated in fp64 on the operands the kernels receive: activations drawn in the storage dtype, Wpos,
Wred and the positional table rounded as the weight shadows and the table copy round them.

Metrics are module_parity's: activation-shaped tensors (elem, worst per-sample rel-L2), parameter-style sums (rel-L2, max-abs over max-abs).
A tensor that is analytically zero (T = 1: one key, so dS = 0 and with it dq, dk, du, dvb, dposp, dWpos) is measured as max |got| over
max |dv|, the size of the operator's gradients: what is left there is the rounding of o (delta = dO . o against dP = dO . v), eps of the storage
dtype times that size.

Bounds
  f32: elem <= 2e-4 for outputs and input gradients, parameter-style sums within 1e-3 of the tensor's max and 1e-3 rel-L2 (module_parity's
       gradient rule); zero: 2e-4.
  bf16: BF16_BOUND below, 2x the largest value observed on the MI355X per tensor over all of its cases, no rel-L2 above 0.03
        (the cap is not reached: the largest rel-L2 bound is 0.011).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import module_parity as MP
from oracle import rng
from oracle import squeezeformer_torch_oracle as S

# (B, H, T, dh): the smallest shapes that reach each tiling edge of the relattn_len_* kernels (RL_QB = 64 rows per workgroup, RL_KT = 32 per chunk)
RELATTN_CASES = [(2, 2, 1, 8), (2, 3, 31, 16), (1, 2, 33, 8), (2, 2, 64, 32), (2, 2, 65, 64), (3, 4, 97, 32), (1, 2, 130, 16)]
SUB_CASES = [(1, 7, 7, 8), (2, 30, 16, 16), (3, 33, 23, 24), (2, 131, 80, 256)]       # (B, T0, F, d)
TRED_CASES = [(2, 7, 16), (2, 8, 24), (3, 37, 64), (2, 98, 512)]                      # (B, Tin, d)
SITE = 5
RATE = 0.2

ACT = ("o", "lse", "dq", "dk", "dv", "sub", "dx", "red", "dh")
PARAM = ("du", "dvb", "dposp", "dWpos", "dw1", "db1", "dw2", "db2", "dconv_w", "dconv_b", "dWred", "dbred")

# 2 x the largest error observed on the MI355X over every bf16 case of tests/test_ops_r4_gpu.py, per tensor (DESIGN.md §2 tabulates the observed
# values): activations (elem, l2), parameter-style sums (l2, max), zero (analytically zero tensors, over max |dv|).  lse, dx, dw1, db1, dw2,
# db2 and dbred are fp32 arithmetic on fp32 (or exactly representable bf16) operands in the bf16 run too: their figure is fp32 rounding, which
# depends on the draw, so the larger of the f32 and the bf16 run's observation is doubled for them (1e-7 ... 3e-6; a new summation order
# moves these figures: measure again rather than widen).
BF16_BOUND = {
    "o": dict(elem=0.0062, l2=0.0037),
    "lse": dict(elem=1.8e-07, l2=1.5e-07),
    "dq": dict(elem=0.038, l2=0.0062),
    "dk": dict(elem=0.015, l2=0.0041),
    "dv": dict(elem=0.0065, l2=0.0043),
    "du": dict(l2=0.0025, max=0.0027),
    "dvb": dict(l2=0.0071, max=0.0086),
    "dposp": dict(l2=0.0017, max=0.0026),
    "dWpos": dict(l2=0.011, max=0.008),
    "zero": dict(zero=0.0018),
    "sub": dict(elem=0.0065, l2=0.0039),
    "dx": dict(elem=2.6e-06, l2=5.7e-07),
    "dw1": dict(l2=2e-07, max=2.8e-07),
    "db1": dict(l2=3e-07, max=4.6e-07),
    "dw2": dict(l2=2.1e-07, max=2.5e-07),
    "db2": dict(l2=1.8e-07, max=1.9e-07),
    "red": dict(elem=0.013, l2=0.0067),
    "dh": dict(elem=0.031, l2=0.0061),
    "dconv_w": dict(l2=0.005, max=0.0051),
    "dconv_b": dict(l2=0.0092, max=0.0092),
    "dWred": dict(l2=0.005, max=0.0062),
    "dbred": dict(l2=1.6e-07, max=2.6e-07),
}
assert all(b.get("l2", 0.0) <= MP.BF16_CAP for b in BF16_BOUND.values())


def bounds(dtype):
    if dtype == "bf16":
        return BF16_BOUND
    out = {n: dict(elem=MP.F32_T) for n in ACT}
    out.update({n: dict(l2=MP.F32_GRAD_MAX, max=MP.F32_GRAD_MAX) for n in PARAM})
    out["zero"] = dict(zero=MP.F32_T)
    return out


def compare(got, ref, bound, rows, alts=(), names=None):
    """Every tensor of `ref` (or `names`) -> (observed {"name.quantity": value}, failures [text]).  alts: further references spanning an
    interval (a ReLU derivative fp64 cannot decide, see subsample_reference)."""
    obs, bad = {}, []

    def see(n, q, v):
        obs[f"{n}.{q}"] = v
        b = bound.get(n, {}).get(q)
        if b is not None and not v <= b:
            bad.append(f"{n}: {q} {v:.3e} > {b:.3e}")

    scale = float(np.abs(ref["dv"]).max()) if "dv" in ref else None
    for n in names or [k for k in ref if k in ACT or k in PARAM]:
        g, r = np.asarray(got[n], np.float64), np.asarray(ref[n], np.float64)
        assert g.shape == r.shape, (n, g.shape, r.shape)
        assert np.isfinite(g).all(), f"{n} is not finite"
        if scale is not None and np.abs(r).max() < 1e-9 * scale:
            v = float(np.abs(g).max() / scale)
            obs[f"{n}.zero"] = v
            if not v <= bound["zero"]["zero"]:
                bad.append(f"{n}: analytically zero, max |got| / max |dv| {v:.3e} > {bound['zero']['zero']:.3e}")
            continue
        al = [a[n] for a in alts]
        if n in ACT:
            e, l2 = MP.act_metrics(g, r, al)
            see(n, "elem", e); see(n, "l2", l2)
        else:
            l2, mx, _ = MP.grad_metrics(g, r, rows, al)
            see(n, "l2", l2); see(n, "max", mx)
    return obs, bad


def _t64(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))
    return t.requires_grad_(True) if grad else t


def _rms(a):
    return float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2)))


# ------------------------------------------------------------------ relative-position attention
@functools.lru_cache(maxsize=None)
def relattn_inputs(case, dtype):
    """q, k, v, dO ~ N(0, 1) in the storage dtype; u, vb ~ N(0, 0.5^2); the reference's table; Wpos ([in, out]) scaled so that pos_proj of the
    table has unit variance: the scores over sqrt(dh) are O(1) and the softmax is not flat (a flat softmax would hide a wrong shift)."""
    B, H, T, dh = case
    d = H * dh
    g = np.random.default_rng([11, B, H, T, dh])
    q, k, v, dO = (MP.round_to(g.standard_normal((B, T, d)), dtype) for _ in range(4))
    u, vb = ((0.5 * g.standard_normal(d)).astype(np.float32) for _ in range(2))
    pe = S.rel_positional_encoding(T, d)[0].numpy().astype(np.float32)
    W0 = g.standard_normal((d, d))
    Wpos = (W0 / _rms(MP.round_to(pe, dtype).astype(np.float64) @ W0)).astype(np.float32)
    return dict(q=q, k=k, v=v, dO=dO, u=u, vb=vb, pe=pe, Wpos=Wpos)


def attn_mask(case, seed, rate, no_head=False):
    """the multiplicative mask [B, H, T, T] of the attention-probability site: row key (b*H + h)*T + i, column j"""
    B, H, T, _ = case
    if rate <= 0:
        return None
    if no_head:      # a kernel keying the rows by b*T + i: every head of a sample draws the same mask
        return torch.from_numpy(rng.scaled_mask_attn(seed, SITE, B * T, T, rate, np.float64).reshape(B, 1, T, T)).expand(B, H, T, T)
    return torch.from_numpy(rng.scaled_mask_attn(seed, SITE, B * H * T, T, rate, np.float64).reshape(B, H, T, T))


def dropout_seed(case, rate, seed=4242):
    """the first seed >= `seed` whose mask drops between 10 % and 30 % of the probabilities (T = 1 has four of them)"""
    for s in range(seed, seed + 4096):
        z = float((attn_mask(case, s, rate) == 0).double().mean())
        if 0.10 <= z <= 0.30:
            return s
    raise AssertionError("no seed with 10 % .. 30 % dropped")


def _scores_row_off(q, k, posp, u, vb, heads):
    """rel_attention_scores with the table read one row off, in the closed form: key j of query i reads row T-i+j; the row past the table's end
    reads as zero (the kernels' bounds check)"""
    B, T, d = q.shape
    dh = d // heads
    qh = q.view(B, T, heads, dh)
    kh = k.view(B, T, heads, dh).permute(0, 2, 1, 3)
    pos = posp.reshape(B, -1, heads, dh)
    content = torch.matmul((qh + u.view(heads, dh)).transpose(1, 2), kh.transpose(2, 3))
    raw = torch.matmul((qh + vb.view(heads, dh)).transpose(1, 2), pos.permute(0, 2, 3, 1))
    raw = torch.cat([raw, raw.new_zeros(B, heads, T, 1)], dim=-1)
    i = torch.arange(T).unsqueeze(1)
    j = torch.arange(T).unsqueeze(0)
    return (content + raw[:, :, i, T - i + j]) / math.sqrt(dh)


@functools.lru_cache(maxsize=None)
def relattn_reference(case, dtype, seed, rate, mut=None):
    """fp64 o, lse, dq, dk, dv, du, dvb, dposp, dWpos.  mut None: oracle.rel_attention (the reference's relative_shift) under autograd.  mut a
    tuple: the flash-style restatement the kernels follow (P from the scores, dS = P * (dP - delta), the score graph differentiated by
    autograd), with the named mistakes switched on; () restates the oracle (tests/test_r4_mutants.py checks that)."""
    B, H, T, dh = case
    d = H * dh
    inp = relattn_inputs(case, dtype)
    q, k, v, u, vb = (_t64(inp[n], True) for n in ("q", "k", "v", "u", "vb"))
    dO = _t64(inp["dO"])
    pe = _t64(MP.round_to(inp["pe"], dtype))
    W = _t64(MP.round_to(inp["Wpos"], dtype), mut is None)
    if mut is None:
        posp = pe @ W
        posp.retain_grad()
        sc = S.rel_attention_scores(q, k, posp, u, vb, H)
        o = S.rel_attention(q, k, v, posp, u, vb, H, attn_mask(case, seed, rate))
        o.backward(dO)
        return dict(o=o.detach().numpy(), lse=torch.logsumexp(sc.detach(), -1).numpy(), dq=q.grad.numpy(), dk=k.grad.numpy(), dv=v.grad.numpy(),
                    du=u.grad.numpy(), dvb=vb.grad.numpy(), dposp=posp.grad.numpy(), dWpos=W.grad.numpy())
    posb = (pe @ W).unsqueeze(0).repeat(B, 1, 1).requires_grad_(True)          # one table per sample: the batch sum of dposp is explicit
    cu, cv = (vb, u) if "swap_uv" in mut else (u, vb)                          # (content bias, positional bias)
    sc = (_scores_row_off if "row_off" in mut else S.rel_attention_scores)(q, k, posb, cu, cv, H)
    mask = attn_mask(case, seed, rate, no_head="mask_no_head" in mut)
    with torch.no_grad():
        heads = lambda t: t.view(B, T, H, dh).permute(0, 2, 1, 3)
        P = torch.softmax(sc, -1)
        Pd = P if mask is None else P * mask
        vh, gh = heads(v), heads(dO)
        oh = Pd @ vh
        dP = gh @ vh.transpose(2, 3)
        if mask is not None and "mask_not_in_bwd" not in mut:
            dP = dP * mask
        delta = (gh * (P @ vh if "delta_undropped" in mut else oh)).sum(-1, keepdim=True)
        dS = P * (dP - delta)
        dv = (Pd.transpose(2, 3) @ gh).permute(0, 2, 1, 3).reshape(B, T, d)
    sc.backward(dS)
    dposp = posb.grad[0] if "dposp_batch0" in mut else posb.grad.sum(0)
    du = cu.grad * (math.sqrt(dh) if "du_no_scale" in mut else 1.0)
    return dict(o=oh.permute(0, 2, 1, 3).reshape(B, T, d).numpy(), lse=torch.logsumexp(sc.detach(), -1).numpy(), dq=q.grad.numpy(), dk=k.grad.numpy(), dv=dv.numpy(),
                du=du.numpy(), dvb=cv.grad.numpy(), dposp=dposp.numpy(), dWpos=(pe.t() @ dposp).numpy())


# ------------------------------------------------------------------ DepthwiseConv2dSubsampling
def sub_dims(T0, Fin):
    T1, F1 = (T0 - 3) // 2 + 1, (Fin - 3) // 2 + 1
    return T1, F1, (T1 - 3) // 2 + 1, (F1 - 3) // 2 + 1


@functools.lru_cache(maxsize=None)
def subsample_inputs(case, dtype):
    B, T0, Fin, d = case
    _, _, T2, F2 = sub_dims(T0, Fin)
    g = np.random.default_rng([12, B, T0, Fin, d])
    return dict(x=g.standard_normal((B, T0, Fin)).astype(np.float32),
                w1=(g.standard_normal((d, 9)) / 3).astype(np.float32), b1=(0.1 * g.standard_normal(d)).astype(np.float32),
                w2=(g.standard_normal((d, 9)) / 3).astype(np.float32), b2=(0.1 * g.standard_normal(d)).astype(np.float32),
                dsub=MP.round_to(g.standard_normal((B * T2, d * F2)), dtype))


def _relu_at(z, shift):
    """relu(z); shift given: the same values, the derivative taken as 1 where z exceeds `shift` instead of 0 (module_parity.head_shifted)"""
    return torch.relu(z) if shift is None else torch.relu(z).detach() + (z - z.detach()) * (z.detach() > shift)


@functools.lru_cache(maxsize=None)
def subsample_reference(case, dtype, mut=None):
    """fp64 sub, dx, dw1, db1, dw2, db2 and `alts`.  mut None: oracle.conv2d_subsampling under autograd; a tuple: the restatement below.
    Each ReLU has no derivative at 0 and some of the pre-activations lie closer to 0 than fp32 accumulation resolves (|z| < tau = 2e-5 rms(z): 9
    products summed in fp32 by the kernel), so fp64 and the kernels may take different sides there, each a whole term of a gradient: two more
    backward passes switch both derivatives at +tau and at -tau, and a compared value is measured against the interval the three span
    (property (b)).  No element is left out."""
    B, T0, Fin, d = case
    inp = subsample_inputs(case, dtype)
    mut_ = mut or ()

    def run(sign):
        x, w1, b1, w2, b2 = (_t64(inp[n], True) for n in ("x", "w1", "b1", "w2", "b2"))
        dsub = _t64(inp["dsub"])
        if mut is None and sign == 0:
            sub = S.conv2d_subsampling(x, {"conv_subsample.sequential.0.weight": w1.view(d, 1, 3, 3), "conv_subsample.sequential.0.bias": b1,
                                           "conv_subsample.sequential.2.conv.weight": w2.view(d, 1, 3, 3), "conv_subsample.sequential.2.conv.bias": b2})
        else:
            z1 = F.conv2d(x.unsqueeze(1), w1.view(d, 1, 3, 3), b1, stride=2)
            y1 = _relu_at(z1, sign * 2e-5 * float(z1.detach().pow(2).mean().sqrt()) if sign else None)
            k2 = w2.view(d, 1, 3, 3)
            z2 = F.conv2d(y1, k2.transpose(2, 3) if "w2_transposed" in mut_ else k2, b2, stride=2, groups=d)
            if "gate_on_dsub" in mut_:       # the backward gating on the sign of the incoming gradient instead of the output's
                gz = dsub.view(B, z2.shape[2], d, z2.shape[3]).permute(0, 2, 1, 3)
                y2 = torch.relu(z2).detach() + (z2 - z2.detach()) * (gz > 0)
            else:
                y2 = _relu_at(z2, sign * 2e-5 * float(z2.detach().pow(2).mean().sqrt()) if sign else None)
            sub = y2.permute(0, 2, 1, 3).contiguous().view(B, y2.shape[2], d * y2.shape[3])
        sub.reshape(dsub.shape).backward(dsub)
        return dict(sub=sub.detach().numpy().reshape(dsub.shape), dx=x.grad.numpy(), dw1=w1.grad.numpy(), db1=b1.grad.numpy(), dw2=w2.grad.numpy(), db2=b2.grad.numpy())

    out = run(0)
    out["alts"] = [run(1), run(-1)] if mut is None else []
    return out


# ------------------------------------------------------------------ TimeReductionLayer + time_reduction_proj
def tred_dims(Tin, d):
    Fr = (d - 1) // 2
    return (Tin - 3) // 2 + 1, Fr, (Fr + 7) // 8 * 8


@functools.lru_cache(maxsize=None)
def tred_inputs(case, dtype):
    B, Tin, d = case
    Tr, Fr, _ = tred_dims(Tin, d)
    g = np.random.default_rng([13, B, Tin, d])
    return dict(h=MP.round_to(g.standard_normal((B, Tin, d)), dtype), conv_w=(g.standard_normal(9) / 3).astype(np.float32),
                conv_b=(0.1 * g.standard_normal(1)).astype(np.float32), Wred=(g.standard_normal((Fr, d)) / Fr ** 0.5).astype(np.float32),
                bred=(0.1 * g.standard_normal(d)).astype(np.float32), dred=MP.round_to(g.standard_normal((B * Tr, d)), dtype),
                extra=MP.round_to(g.standard_normal((B, Tin, d)), dtype))


@functools.lru_cache(maxsize=None)
def tred_reference(case, dtype, with_extra, mut=()):
    """fp64 red, dh (= extra + the input gradient), dconv_w, dconv_b, dWred, dbred through oracle.time_reduction and the Linear that follows it
    in oracle.encoder"""
    B, Tin, d = case
    inp = tred_inputs(case, dtype)
    h, cw, cb, bred = (_t64(inp[n], True) for n in ("h", "conv_w", "conv_b", "bred"))
    Wred = _t64(MP.round_to(inp["Wred"], dtype), True)
    k = cw.view(1, 1, 3, 3)
    y = S.time_reduction(h, {"time_reduction_layer.sequential.0.conv.weight": k.transpose(2, 3) if "w_transposed" in mut else k,
                             "time_reduction_layer.sequential.0.conv.bias": cb})
    red = (y @ Wred + bred).reshape(-1, d)
    red.backward(_t64(inp["dred"]))
    dh = h.grad.numpy()
    if with_extra and "ignore_extra" not in mut:
        dh = dh + inp["extra"].astype(np.float64)
    return dict(red=red.detach().numpy(), dh=dh, dconv_w=cw.grad.numpy(), dconv_b=cb.grad.numpy(), dWred=Wred.grad.numpy(), dbred=bred.grad.numpy())
