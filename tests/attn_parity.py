"""Helpers of tests/test_attn_gpu.py and tests/test_attn_mutants.py: the cases, the inputs, the fp64 reference, the metrics and the bounds of the
training attention operators (attention.hip's lane-split kernels, attention_mfma.hip's and attention_bwd_mfma.hip's MFMA kernels) through ishara_op_attn_fwd / _bwd.

Reference: test_ops_gpu._attn_ref (softmax(q.k^T * scale) * mask . v on the packed head-major qkv) in fp64 under autograd, on the operands the
kernel receives (drawn in the storage dtype); the dropout mask is oracle/rng.py's scaled_mask_attn with row key (b*H + h)*T + i.  dqkv is
compared split into dq, dk, dv; lse = log sum exp(scale * s); delta = rowsum(dO o o) is compared against the kernel's own o (the tests do that).

Metrics are module_parity's act_metrics: elem = max |err| / (rms(ref) + |ref|) and the worst per-sample relative L2; a tensor that is
analytically zero (T = 1: dq, dk; q = 0: dk) is measured as max |got| / max |dv| ("zero").  No element is left out.

Bounds
  f32 (lane-split): elem <= 2e-4 for every tensor, zero 2e-4 (the operator bound, as in r4_parity).
  bf16: BF16_BOUND below: to be 2x the largest value observed on the MI355X per tensor over all of its cases and routes; until
        that run is recorded, the bounds the formats give: rel-L2 <= module_parity.BF16_CAP = 0.03 on every tensor, lse and delta at the f32 bound.  A score regime that exceeded them has, once the excess was shown to be rounding, a
        bound of its own in BF16_REGIME_BOUND.  restate(ideal_bf16=True) restates the MFMA algorithm in fp64 with its bf16 roundings: the CPU test holds
        it inside the same bounds (they are not below what the format allows), and a GPU figure far above its figure is a finding.
"""
import collections
import functools
import math

import numpy as np
import torch

import module_parity as MP
from oracle import rng
from test_ops_gpu import _attn_ref

SITE = 7
RATE = 0.2
KC = {"mfma": 64, "lane": 32}       # keys per staged chunk (AF_KC, ATT_KC)
QB = {"mfma": 128, "lane": 64}      # queries per workgroup (AF_QB, 64)
TENSORS = ("o", "lse", "dq", "dk", "dv", "delta")
ROUNDED = ("o", "dq", "dk", "dv")   # stored in the storage dtype
F32, BF16 = 0, 1
DROP, BITS, HEAD_MAJOR = 1, 2, 4    # flag bits of ishara_debug_attn_kernel_name
TWO_PASS = 1 << 16                  # ishara_debug_force_regstage: the two-kernel attention backward instead of the one-pass kernel

# route: "mfma" (impl 1 / 2, bf16) or "lane" (impl 0); dm: 0 no dropout, 1 hashed again in the backward (impl 2), 2 cached keep bits (impl 1);
# two_pass: the two-kernel MFMA backward forced (bit 16 of ishara_debug_force_regstage); regime: see inputs()
Case = collections.namedtuple("Case", "route dtype B H T dh rate dm two_pass regime")


def case_id(c):
    return f"{c.route}-{c.dtype}-B{c.B}-H{c.H}-T{c.T}-dh{c.dh}-r{c.rate:g}-dm{c.dm}{'-2pass' if c.two_pass else ''}-{c.regime}"


def shape(c):
    return (c.B, c.H, c.T, c.dh)


def impl(c):
    return 0 if c.route == "lane" else (2 if c.dm == 1 else 1)


def bwd_kernel(lib, c):
    """the backward instantiation launch_attn_bwd runs for the case as ishara_op_attn_bwd calls it (head-major dqkv; impl 1: the keep-bit buffer
    given), read from the route itself (ishara_debug_attn_kernel_name: host only, nothing is launched); "" for a refused call"""
    flags = (DROP if c.rate > 0 and int(rng.threshold8(c.rate)) else 0) | (BITS if impl(c) == 1 else 0) | HEAD_MAJOR
    lib.ishara_debug_force_regstage(TWO_PASS if c.two_pass else 0)
    try:
        return lib.ishara_debug_attn_kernel_name(BF16 if c.dtype == "bf16" else F32, 1, c.T, c.dh, min(impl(c), 1), flags).decode()
    finally:
        lib.ishara_debug_force_regstage(0)


def writes_delta(lib, c):
    return not bwd_kernel(lib, c).startswith("attn_bwd_fused")


MAIN = "std4"
MFMA_T32 = (8, 56, 64, 72, 120, 128, 136, 184, 192, 200, 248, 256, 264, 376, 384, 392)
MFMA_T64 = (8, 64, 72, 128, 136, 264)
REGIMES = ("std1", "std4", "std12", "q0", "late", "early")


def _mfma_shapes():
    s = [(1, 3, T, 32, False) for T in MFMA_T32]
    s += [(1, 3, T, 32, True) for T in MFMA_T32[:-1]]      # forced where the one-pass kernel is the default: every T but the last
    s += [(1, 3, T, 64, False) for T in MFMA_T64]
    s += [(2, 8, T, 32, False) for T in (136, 264, 392)] + [(2, 8, 136, 64, False)]
    return s


def _cases():
    out = []
    for B, H, T, dh, tp in _mfma_shapes():
        out += [Case("mfma", "bf16", B, H, T, dh, r, dm, tp, MAIN) for r, dm in ((0.0, 0), (RATE, 2), (RATE, 1))]
    out.append(Case("mfma", "bf16", 1, 3, 64, 32, 0.5, 2, False, MAIN))
    lane = [(2, 3, 33, dh) for dh in (8, 16, 24, 32, 48, 64)]
    lane += [(2, 3, T, dh) for dh in (16, 24) for T in (1, 7, 31, 32, 63, 64, 65, 130)] + [(3, 8, 65, 8)]
    for dt in ("f32", "bf16"):
        out += [Case("lane", dt, B, H, T, dh, r, 1 if r else 0, False, MAIN) for B, H, T, dh in lane for r in (0.0, RATE)]
    for reg in REGIMES:
        if reg == MAIN:
            continue
        out += [Case("mfma", "bf16", 1, 3, 136, dh, 0.0, 0, False, reg) for dh in (32, 64)]
        out += [Case("mfma", "bf16", 1, 3, 136, 32, 0.0, 0, True, reg)]
        out += [Case("lane", dt, 2, 3, 65, 16, 0.0, 0, False, reg) for dt in ("f32", "bf16")]
    return out


CASES = _cases()
# thr8 = round(0.001 * 256) = 0: no dropout at all, o and dqkv bit-equal to the rate-0 run
TINY_RATE_CASE = Case("mfma", "bf16", 1, 3, 72, 32, 0.001, 2, False, MAIN)

# Interim bounds, from the formats alone: no MI355X run of tests/test_attn_gpu.py has been recorded yet, so the "2 x observed"
# figures are still missing and no number is invented for them.  What needs no measurement is asserted:
#   o, dq, dk, dv   rel-L2 <= module_parity.BF16_CAP = 0.03, the cap no bf16 bound of this project may exceed.  The ideal bf16 restatement stays
#                   below half of it at every MFMA case and each mistake of tests/test_attn_mutants.py exceeds it by 4.9x or more (both asserted
#                   there).  elem is None = not bounded yet: it is printed and logged (ISHARA_ATTN_LOG).
#   lse, delta      fp32 arithmetic on operands that are exact in bf16 (the row sum is taken before P is rounded; delta is compared against the
#                   kernel's own stored o): the f32 operator bound, elem 2e-4.
#   zero            T = 1 without dropout, q = 0 and the one-key late case leave an exact or fp32-sized zero.  T = 1 with dropout does not:
#                   o = bf16(1.25 v), so dP o D - delta = g . (1.25 v - bf16(1.25 v)), a residue of o's rounding that reaches dq and dk through
#                   dS.  The restatement gives 6.7e-3 of max |dv| at dh 24 (4.0e-3 at dh 16); the bound is 2 x that.
# To be tightened to 2 x the largest figure observed on the MI355X per tensor once the log is in.
BF16_BOUND = {
    "o": dict(elem=None, l2=MP.BF16_CAP),
    "lse": dict(elem=MP.F32_T, l2=MP.BF16_CAP),
    "dq": dict(elem=None, l2=MP.BF16_CAP),
    "dk": dict(elem=None, l2=MP.BF16_CAP),
    "dv": dict(elem=None, l2=MP.BF16_CAP),
    "delta": dict(elem=MP.F32_T, l2=MP.BF16_CAP),
    "zero": dict(zero=1.4e-2),
}
BF16_REGIME_BOUND = {}      # regime -> {tensor: {quantity: bound}}: overrides of BF16_BOUND for one score regime (none needed unless listed)
assert all(0.0 < b["l2"] <= MP.BF16_CAP for bb in [BF16_BOUND, *BF16_REGIME_BOUND.values()] for b in bb.values() if "l2" in b)


def bounds(c):
    if c.dtype == "bf16":
        out = {n: dict(b) for n, b in BF16_BOUND.items()}
        for n, b in BF16_REGIME_BOUND.get(c.regime, {}).items():
            out[n].update(b)
        return out
    out = {n: dict(elem=MP.F32_T) for n in TENSORS}
    out["zero"] = dict(zero=MP.F32_T)
    return out


def compare(got, ref, bound, names=None):
    """every tensor of `names` (default: all of ref) -> (observed {"name.quantity": value}, failures [text])"""
    obs, bad = {}, []
    scale = float(np.abs(ref["dv"]).max())
    for n in names or [k for k in TENSORS if k in ref]:
        g, r = np.asarray(got[n], np.float64), np.asarray(ref[n], np.float64)
        assert g.shape == r.shape, (n, g.shape, r.shape)
        if not np.isfinite(g).all():
            bad.append(f"{n}: {int((~np.isfinite(g)).sum())} of {g.size} elements are not finite (never written, or NaN)")
            continue
        if n in ("dq", "dk") and np.abs(r).max() < 1e-9 * scale:
            v = float(np.abs(g).max() / scale)
            obs[f"{n}.zero"] = v
            b = bound["zero"]["zero"]
            if b is not None and not v <= b:
                bad.append(f"{n}: analytically zero, max |got| / max |dv| {v:.3e} > {b:.3e}")
            continue
        e, l2 = MP.act_metrics(g, r)
        for q, v in (("elem", e), ("l2", l2)):
            obs[f"{n}.{q}"] = v
            b = bound.get(n, {}).get(q)
            if b is not None and not v <= b:
                bad.append(f"{n}: {q} {v:.3e} > {b:.3e}")
    return obs, bad


# ------------------------------------------------------------------ inputs
LEVEL_GAP = 50.0      # late / early: the score offset between the keys of one chunk and of the next


def scale_of(c):
    return {"std1": 1.0, "std12": 12.0}.get(c.regime, 4.0) * c.dh ** -0.5


@functools.lru_cache(maxsize=None)
def _inputs(shp, dtype, regime, kc):
    B, H, T, dh = shp
    g = np.random.default_rng([21, B, H, T, dh])
    q, k, v = (g.standard_normal((B, T, H, dh)) for _ in range(3))
    dO = g.standard_normal((B * T, H * dh))
    if regime == "q0":
        q = np.zeros_like(q)
    elif regime in ("late", "early"):
        # along the unit vector u every query carries a and the keys of chunk n carry 2 n (late) or 2 (last - n) (early), nothing else of q or k
        # lies along u: scale * q.k = the std4 scores + LEVEL_GAP * n.  Every chunk raises the running maximum by about 50 (late), or the first
        # chunk holds it and the third lies 100 below, where exp underflows in fp32 (early).  k keeps its size (2 n against |k| = sqrt(dh)) and dS
        # sums to zero over a row, so no gradient is a small difference of large terms: the regime is as well conditioned as std4.
        u = np.ones(dh) / math.sqrt(dh)
        a = LEVEL_GAP * math.sqrt(dh) / (4.0 * 2.0)
        lev = np.arange(T) // kc
        lev = lev if regime == "late" else lev.max() - lev
        q = q - (q @ u)[..., None] * u + a * u
        k = k - (k @ u)[..., None] * u + (2.0 * lev)[None, :, None, None] * u
    qkv = np.concatenate([q, k, v], axis=-1).reshape(B * T, 3 * H * dh)      # head-major packing: per head q | k | v
    return MP.round_to(qkv, dtype), MP.round_to(dO, dtype)


def inputs(c):
    """(qkv [B*T, 3*H*dh] head-major, dO [B*T, H*dh]) fp32 arrays holding storage-dtype values.  Regimes: std1 / std4 / std12 — q, k ~ N(0, 1)
    and the scale 1, 4, 12 over sqrt(dh) (the model's, test_attention's, a near one-hot softmax); q0 — q = 0, a uniform softmax; late / early — the
    largest score of every query in the last / first chunk of the route's KC keys (scale as std4)."""
    return _inputs(shape(c), c.dtype, c.regime, KC[c.route])


def mask_of(shp, seed, rate, variant=None, qb=128):
    """the multiplicative dropout mask [B, H, T, T] (None without dropout).  variant: "no_head" rows keyed b*T + i, "qblock0" the rows of query
    block 0 (`qb` queries) used for every block"""
    B, H, T, _ = shp
    if rate <= 0 or int(rng.threshold8(rate)) == 0:
        return None
    if variant == "no_head":
        return torch.from_numpy(rng.scaled_mask_attn(seed, SITE, B * T, T, rate, np.float64).reshape(B, 1, T, T)).expand(B, H, T, T)
    m = torch.from_numpy(rng.scaled_mask_attn(seed, SITE, B * H * T, T, rate, np.float64).reshape(B, H, T, T))
    if variant == "qblock0":
        m = m[:, :, torch.arange(T) % qb]
    return m


def mask_share_range(rate):
    """the share of zeros a mask of at least 4096 elements must show: 10 .. 30 % at rate 0.2, the quantised rate +- 10 points otherwise"""
    want = int(rng.threshold8(rate)) / 256.0
    return (0.10, 0.30) if rate == RATE else (want - 0.10, want + 0.10)


@functools.lru_cache(maxsize=None)
def dropout_seed(shp, rate, seed=4242):
    """the first seed >= `seed` whose mask drops a share inside mask_share_range; masks of fewer than 4096 elements take `seed`"""
    B, H, T, _ = shp
    if rate <= 0 or int(rng.threshold8(rate)) == 0 or B * H * T * T < 4096:
        return seed
    lo, hi = mask_share_range(rate)
    for s in range(seed, seed + 64):
        if lo <= float((mask_of(shp, s, rate) == 0).double().mean()) <= hi:
            return s
    raise AssertionError("no seed whose mask drops the wanted share")


def seed_of(c):
    return dropout_seed(shape(c), c.rate)


def split(dqkv, shp):
    """packed head-major dqkv [B*T, 3*H*dh] -> dq, dk, dv [B, T, H, dh]"""
    B, H, T, dh = shp
    a = np.asarray(dqkv).reshape(B, T, H, 3, dh)
    return a[:, :, :, 0], a[:, :, :, 1], a[:, :, :, 2]


def delta_from(o, dO, shp):
    """rowsum(dO o o) per (b, h, query), [B, H, T], in fp64 from the given o"""
    B, H, T, dh = shp
    p = np.asarray(o, np.float64).reshape(B, T, H, dh) * np.asarray(dO, np.float64).reshape(B, T, H, dh)
    return p.sum(-1).transpose(0, 2, 1)


# ------------------------------------------------------------------ fp64 reference
@functools.lru_cache(maxsize=256)
def _reference(shp, dtype, regime, kc, rate, seed, scale):
    B, H, T, dh = shp
    qkv, dO = _inputs(shp, dtype, regime, kc)
    x = torch.from_numpy(qkv.astype(np.float64)).requires_grad_(True)
    o = _attn_ref(x, B, H, T, dh, scale, mask_of(shp, seed, rate))
    o.backward(torch.from_numpy(dO.astype(np.float64)))
    with torch.no_grad():
        q4 = x.view(B, T, H, 3 * dh).permute(0, 2, 1, 3)
        lse = torch.logsumexp(q4[..., :dh] @ q4[..., dh:2 * dh].transpose(-1, -2) * scale, -1)
    dq, dk, dv = split(x.grad.numpy(), shp)
    out = dict(o=o.detach().numpy().reshape(B, T, H * dh), lse=lse.numpy(), dq=dq, dk=dk, dv=dv)
    out["delta"] = delta_from(out["o"], dO, shp)
    for a in out.values():
        a.setflags(write=False)
    return out


def reference(c):
    """fp64 o [B, T, d], lse [B, H, T], dq, dk, dv [B, T, H, dh], delta [B, H, T] (from the reference's own o)"""
    return _reference(shape(c), c.dtype, c.regime, KC[c.route], c.rate, seed_of(c), scale_of(c))


# ------------------------------------------------------------------ the algorithm restated: mistakes, and the bf16 roundings
def _bf(t, on):
    return t.to(torch.float32).to(torch.bfloat16).double() if on else t


def restate(c, mut=(), ideal_bf16=False):
    """The flash algorithm the kernels follow, in fp64: the online softmax over chunks of KC keys, P from the scores and lse in the backward,
    dS = P o (dP o D - delta) * scale.  mut: the mistakes of tests/test_attn_mutants.py, by name.  ideal_bf16: the MFMA kernels' roundings — the
    unnormalised (dropped) P to bf16 before P.V with the row sum taken unrounded, o to bf16, delta from that o, P o D and dS to bf16 before the
    backward products, dq, dk, dv to bf16 — every sum exact."""
    B, H, T, dh = shape(c)
    kc, qb = KC[c.route], QB[c.route]
    scale, seed = scale_of(c), seed_of(c)
    qkv, dO = inputs(c)
    x = torch.from_numpy(qkv.astype(np.float64)).view(B, T, H, 3 * dh).permute(0, 2, 1, 3)
    q, k, v = x[..., :dh], x[..., dh:2 * dh], x[..., 2 * dh:]
    g = torch.from_numpy(dO.astype(np.float64)).view(B, T, H, dh).permute(0, 2, 1, 3)
    mask = mask_of(shape(c), seed, c.rate, "no_head" if "mask_no_head" in mut else "qblock0" if "mask_qblock0" in mut else None, qb)
    keep_scale = 1.0 if mask is None else float(mask.max())
    keep = None if mask is None else (mask != 0).double()
    s = q @ k.transpose(-1, -2) * scale
    pad = (-T) % kc
    dup = pad if ("keys_past_T_unmasked" in mut or "vt_past_T_not_zeroed" in mut) else 0      # key T-1 (the clamped load) counted `pad` times more
    # ---- forward: online softmax, chunk by chunk
    m = torch.full((B, H, T, 1), -1e30, dtype=torch.float64)
    l = torch.zeros(B, H, T, 1, dtype=torch.float64)
    acc = torch.zeros(B, H, T, dh, dtype=torch.float64)
    for k0 in range(0, T, kc):
        sc = s[..., k0:k0 + kc]
        mn = torch.maximum(m, sc.max(-1, keepdim=True).values)
        corr = torch.exp(m - mn)
        p = torch.exp(sc - mn)
        l = l * corr + p.sum(-1, keepdim=True)
        pd = p if keep is None else p * keep[..., k0:k0 + kc]
        acc = (acc if "acc_not_rescaled" in mut else acc * corr) + _bf(pd, ideal_bf16) @ v[..., k0:k0 + kc, :]
        if dup and k0 + kc > T:
            pl = torch.exp(s[..., T - 1:T] - mn)
            l = l + dup * pl
            if "vt_past_T_not_zeroed" in mut:      # V^T row e read past its T keys runs into row e + 1 (the last row: into what follows, taken as 0)
                vt = torch.cat([v.transpose(-1, -2).reshape(B, H, dh * T), torch.zeros(B, H, pad, dtype=torch.float64)], -1)
                idx = (torch.arange(dh)[:, None] * T + T + torch.arange(pad)[None, :]).reshape(-1)
                acc = acc + pl * vt[..., idx].reshape(B, H, 1, dh, pad).sum(-1)
        m = mn
    o = _bf(acc / l * (1.0 if "o_without_keep_scale" in mut else keep_scale), ideal_bf16)
    lse = torch.log(l) + (0.0 if "lse_without_max" in mut else m)
    # ---- backward
    P = torch.exp(s - lse)
    D = mask if mask is not None else torch.ones(())
    o_for_delta = (P @ v) if "delta_from_undropped_o" in mut else o
    delta = (g * o_for_delta).sum(-1, keepdim=True)
    dP = g @ v.transpose(-1, -2)
    if "mask_not_in_dP" not in mut:
        dP = dP * D
    dS = _bf(P * (dP - delta) * (1.0 if "dS_without_scale" in mut else scale), ideal_bf16)
    PD = _bf(P if "mask_not_in_dV" in mut else P * D, ideal_bf16)
    dv = _bf(PD.transpose(-1, -2) @ g, ideal_bf16)
    dq = _bf(dS @ k, ideal_bf16)
    nq = qb if "dk_first_query_block_only" in mut else T
    dk = _bf(dS[..., :nq, :].transpose(-1, -2) @ q[..., :nq, :], ideal_bf16)
    if "q_k_columns_swapped" in mut:
        dq, dk = dk, dq
    tok = lambda t: t.permute(0, 2, 1, 3).contiguous().numpy()      # [B, H, T, dh] -> [B, T, H, dh]
    return dict(o=tok(o).reshape(B, T, H * dh), lse=lse[..., 0].numpy(), dq=tok(dq), dk=tok(dk), dv=tok(dv), delta=delta[..., 0].numpy())
