"""Helpers of tests/test_relattn_len.py, test_relattn_len_mutants.py and test_relattn_len_gpu.py: the cases, the fp64 references and the bounds of
the Squeezeformer family's relative-position attention WITH PER-CLIP LENGTHS (csrc/relattn_len.hip; SqueezeformerEncoder(mask_padding=True)).

Operator level.  The inputs are r4_parity.relattn_inputs; the reference is oracle.squeezeformer_torch_oracle.rel_attention_scores, then what
RelativeMultiHeadAttention.forward does with its mask (attention.py:75-92): masked_fill(key >= n[b], -1e9), softmax, dropout mask, context, under
autograd.  The n[b] = 0 convention (o = 0, no gradient through the clip) is applied explicitly: the fill alone would give a uniform average of the
padding there.  `mut` a tuple: the flash-style restatement the kernels follow (keys EXCLUDED, P recomputed from the scores and the lse,
dS = P (dP keep - delta)) with switchable mistakes.

Encoder level.  masked_encoder restates SO.encoder / block / rel_mhsa with the mask built from the input lengths by stage_lengths (the reference's
own length arithmetic, clamped), reusing SO's subsampling, time reduction, FFN, convolution module and LayerNorm.

Bounds.  f32: r4_parity.bounds("f32").  bf16: r4_parity.BF16_BOUND; where a tensor of a case exceeds it, 2 x the error of the fp64 restatement
that rounds where the kernels of the route round against the clean reference — computed here, on the CPU, never from a kernel's output — and
no rel-L2 above module_parity.BF16_CAP.  Lane route: o, dq, dk, dv stored in bf16, delta computed from the stored o.  MFMA route (bf16, head dim
32 / 64: MFMA forward, lane backward): also q+u, q+vb, posp and the unnormalised P rounded to bf16 in the forward, and the backward's
P = exp(s - lse) taken from the exact scores against the forward's lse.
"""
import functools
import math

import numpy as np
import torch

import module_parity as MP
import r4_parity as R
from oracle import squeezeformer_torch_oracle as SO

QB, KC = 64, 32      # queries (keys, table rows) per workgroup and keys per LDS chunk of the relattn_len_* kernels (RL_QB, RL_KT)
DEAD_LSE = float(np.float32(1e30))      # ATT_DEAD_LSE: the lse stored for a row with no key

# ((B, H, T, dh), n): a ragged pair per tiling edge of the parent's cases, a dead and a one-key clip, the real stage shapes (T 199 / 99 at T0 = 800), the lane-only head dims, then T at QB-1 / QB and lengths at KC-1, KC, KC+1 (T = QB+1 is (2, 2, 65, 64) above)
OP_CASES = [
    ((2, 2, 64, 32), (64, 37)),
    ((2, 2, 65, 64), (65, 33)),
    ((3, 4, 97, 32), (97, 0, 1)),         # a dead clip and a one-key clip
    ((2, 2, 199, 64), (199, 98)),         # the real stage shape at T0 = 800
    ((2, 2, 99, 64), (48, 99)),
    ((2, 3, 31, 16), (31, 9)),
    ((1, 2, 33, 8), (20,)),
    ((1, 2, 130, 16), (129,)),
    ((2, 2, 63, 32), (31, 63)),
    ((2, 2, 64, 32), (32, 33)),
]
RATES = (0.0, R.RATE)


def case_id(c):
    return "B%d-H%d-T%d-dh%d-n" % c[0] + "_".join(str(v) for v in c[1])


# ------------------------------------------------------------------ stage lengths
def stage_dims(T0):
    T2 = ((T0 - 3) // 2 + 1 - 3) // 2 + 1
    T3 = (T2 - 3) // 2 + 1
    return T2, T3, 2 * T3


def stage_lengths(L, T0):
    """input frames per clip -> (n2, n3, nrec): keys after the conv2d subsampling (convolution.py:68-71), in the reduced layers (:266-268), after
    recovery (encoder.py:162), each clamped to the length the layers run at"""
    T2, T3, Trec = stage_dims(T0)
    clamp = lambda v, hi: min(max(v, 0), hi)
    n2 = [clamp((clamp(int(l), T0) >> 2) - 1, T2) for l in L]
    n3 = [clamp((v >> 1) - 1, T3) for v in n2]
    return n2, n3, [clamp(2 * v, Trec) for v in n3]


# ------------------------------------------------------------------ operator reference
def _allow(case, n, mut=()):
    """[B, 1, T, T] bool: key j of query i takes part"""
    B, H, T, _ = case
    nn = torch.tensor([min(max(int(v), 0), T) for v in n])
    i = torch.arange(T).view(1, T, 1)
    j = torch.arange(T).view(1, 1, T)
    if "len_ignored" in mut:
        a = torch.ones(B, T, T, dtype=torch.bool)
    elif "len_le" in mut:
        a = (j <= nn.view(B, 1, 1)).expand(B, T, T)
    elif "len_on_queries" in mut:
        a = (i < nn.view(B, 1, 1)).expand(B, T, T)
    else:
        a = (j < nn.view(B, 1, 1)).expand(B, T, T)
    return a.unsqueeze(1)


@functools.lru_cache(maxsize=None)
def reference(case, n, dtype, seed, rate, mut=None):
    """fp64 o, lse, dq, dk, dv, du, dvb, dposp, dWpos of the attention with key lengths n.  mut None: the oracle's scores, the reference's -1e9
    fill, autograd.  mut a tuple: the by-hand flash-style restatement with the keys excluded; () restates the oracle.  Mistakes: len_ignored,
    len_le (j <= n), len_on_queries, len_not_in_bwd (P recomputed over every key in the backward), mask_no_head (dropout keyed without the
    head), row_off (the positional window one row off); bf16_storage is no mistake: the stored o is rounded before delta is taken from it."""
    B, H, T, dh = case
    d = H * dh
    inp = R.relattn_inputs(case, dtype)
    q, k, v, u, vb = (R._t64(inp[x], True) for x in ("q", "k", "v", "u", "vb"))
    dO = R._t64(inp["dO"])
    pe = R._t64(MP.round_to(inp["pe"], dtype))
    W = R._t64(MP.round_to(inp["Wpos"], dtype), mut is None)
    live = torch.tensor([1.0 if min(max(int(x), 0), T) > 0 else 0.0 for x in n], dtype=torch.float64).view(B, 1, 1, 1)
    if mut is None:
        posp = pe @ W
        posp.retain_grad()
        sc = SO.rel_attention_scores(q, k, posp, u, vb, H).masked_fill(~_allow(case, n), -1e9)
        attn = torch.softmax(sc, -1) * live                      # n[b] = 0: zeros, not the fill's uniform average
        mask = R.attn_mask(case, seed, rate)
        if mask is not None:
            attn = attn * mask
        o = torch.matmul(attn, v.view(B, T, H, dh).permute(0, 2, 1, 3)).transpose(1, 2).contiguous().view(B, T, d)
        o.backward(dO)
        return dict(o=o.detach().numpy(), lse=torch.logsumexp(sc.detach(), -1).numpy(), dq=q.grad.numpy(), dk=k.grad.numpy(), dv=v.grad.numpy(),
                    du=u.grad.numpy(), dvb=vb.grad.numpy(), dposp=posp.grad.numpy(), dWpos=W.grad.numpy())
    posb = (pe @ W).unsqueeze(0).repeat(B, 1, 1).requires_grad_(True)
    sc = (R._scores_row_off if "row_off" in mut else SO.rel_attention_scores)(q, k, posb, u, vb, H)
    mask = R.attn_mask(case, seed, rate, no_head="mask_no_head" in mut)
    allow = _allow(case, n, mut)
    with torch.no_grad():
        heads = lambda t: t.view(B, T, H, dh).permute(0, 2, 1, 3)
        s = sc.detach().masked_fill(~allow, -math.inf)
        lse = torch.logsumexp(s, -1, keepdim=True)                 # -inf for a row with no key
        dead = torch.isinf(lse)
        lse = lse.masked_fill(dead, DEAD_LSE)
        P = torch.exp(s - lse)                                     # 0 at an excluded key and in a dead row
        Pb = torch.exp(sc.detach() - lse) if "len_not_in_bwd" in mut else P
        Pd = P if mask is None else P * mask
        vh, gh = heads(v), heads(dO)
        if "mfma_fwd" in mut:      # the MFMA forward: q+u, q+vb, posp and the unnormalised P rounded to bf16; the lane backward then recomputes P
            rb = lambda t: torch.from_numpy(MP.round_to(t.numpy(), "bf16").astype(np.float64))      # from the exact scores and THIS lse
            qh = q.detach().view(B, T, H, dh)
            qu_r, qv_r = rb(qh + u.detach().view(H, dh)).transpose(1, 2), rb(qh + vb.detach().view(H, dh)).transpose(1, 2)
            pos_r = rb(posb.detach()).reshape(B, -1, H, dh).permute(0, 2, 3, 1)
            raw = qv_r @ pos_r
            if "row_off" in mut:
                raw = torch.cat([raw, raw.new_zeros(B, H, T, 1)], -1)
            ii, jj = torch.arange(T).unsqueeze(1), torch.arange(T).unsqueeze(0)
            sf = ((qu_r @ heads(k.detach()).transpose(2, 3) + raw[:, :, ii, T - (0 if "row_off" in mut else 1) - ii + jj]) / math.sqrt(dh)).masked_fill(~allow, -math.inf)
            mxf = sf.max(-1, keepdim=True).values
            mxf = mxf.masked_fill(torch.isinf(mxf), 0.0)
            pn = torch.exp(sf - mxf)
            lf = pn.sum(-1, keepdim=True)
            lse = torch.where(lf > 0, mxf + torch.log(lf), torch.full_like(lf, DEAD_LSE))
            Pd = rb(pn if mask is None else pn * (mask != 0)) / lf.clamp_min(1e-300) * (1.0 if mask is None else mask.max())
            Pb = torch.exp(s - lse)
        oh = Pd @ vh
        dP = gh @ vh.transpose(2, 3)
        if mask is not None:
            dP = dP * mask
        o_st = torch.from_numpy(MP.round_to(oh.numpy(), "bf16").astype(np.float64)) if "bf16_storage" in mut else oh
        delta = (gh * o_st).sum(-1, keepdim=True)
        dS = Pb * (dP - delta)
        dv = ((Pb if mask is None else Pb * mask).transpose(2, 3) @ gh).permute(0, 2, 1, 3).reshape(B, T, d)
    sc.backward(dS)
    dposp = posb.grad.sum(0)
    return dict(o=oh.permute(0, 2, 1, 3).reshape(B, T, d).numpy(), lse=lse.squeeze(-1).numpy(), dq=q.grad.numpy(), dk=k.grad.numpy(), dv=dv.numpy(),
                du=u.grad.numpy(), dvb=vb.grad.numpy(), dposp=dposp.numpy(), dWpos=(pe.t() @ dposp).numpy())


def dead_clips(case, n):
    return [b for b, v in enumerate(n) if min(max(int(v), 0), case[2]) == 0]


def without_dead_lse(out, case, n):
    """a copy whose lse of the dead clips is 0: the stored value there is the ATT_DEAD_LSE sentinel (checked by the caller), not a quantity"""
    o = dict(out)
    o["lse"] = np.array(out["lse"], np.float64, copy=True)
    for b in dead_clips(case, n):
        o["lse"][b] = 0.0
    return o


def compare(got, ref, bound, case, n):
    """r4_parity.compare on the tensors with the dead clips' lse taken out, and with the one-key clips' dq and dk measured as what they are:
    analytically zero (P = 1, so dS = 0; what a kernel leaves there is the storage rounding of o in delta = dO . o against dP = dO . v), by
    r4_parity's rule for such tensors, max |got| over max |dv| against the `zero` bound.  The per-sample rel-L2 has no meaning for them."""
    got, ref = without_dead_lse(got, case, n), without_dead_lse(ref, case, n)
    obs, bad = {}, []
    scale = float(np.abs(ref["dv"]).max())
    for b, nb in enumerate(n):
        if min(max(int(nb), 0), case[2]) != 1:
            continue
        for name in ("dq", "dk"):
            assert np.abs(ref[name][b]).max() < 1e-9 * scale, (name, b)
            v = float(np.abs(got[name][b]).max() / scale)
            obs[f"{name}.zero"] = max(v, obs.get(f"{name}.zero", 0.0))
            if not v <= bound["zero"]["zero"]:
                bad.append(f"{name}[{b}]: analytically zero (one key), max |got| / max |dv| {v:.3e} > {bound['zero']['zero']:.3e}")
            got[name], ref[name] = np.array(got[name], np.float64, copy=True), np.array(ref[name], np.float64, copy=True)
            got[name][b] = 0.0
            ref[name][b] = 0.0
    o2, b2 = R.compare(got, ref, bound, case[0] * case[2])
    obs.update(o2)
    return obs, bad + b2


ROUNDED = ("o", "dq", "dk", "dv")      # what a kernel stores in the storage dtype


def rounded(out, dtype):
    return {k: (MP.round_to(v, dtype).astype(np.float64) if k in ROUNDED else v) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def op_bounds(case, n, dtype, seed, rate, mfma=False):
    """r4_parity's bounds; bf16: raised, per quantity, to 2 x the rounding restatement's error where that is larger (see the head).  mfma: the
    route with the MFMA forward, whose restatement also rounds q+u, q+vb, posp and P"""
    base = R.bounds(dtype)
    if dtype != "bf16":
        return base
    ref = reference(case, n, dtype, seed, rate)
    st = rounded(reference(case, n, dtype, seed, rate, mut=("bf16_storage", "mfma_fwd") if mfma else ("bf16_storage",)), dtype)
    obs, _ = compare(st, ref, {"zero": dict(zero=math.inf)}, case, n)
    out = {k: dict(v) for k, v in base.items()}
    for key, val in obs.items():
        name, qn = key.rsplit(".", 1)
        if qn == "zero":
            continue
        if name in out and qn in out[name] and 2 * val > out[name][qn]:
            out[name][qn] = min(2 * val, MP.BF16_CAP) if qn == "l2" else 2 * val
    return out


# ------------------------------------------------------------------ encoder restatement
ENC_CASES = {
    "dh32_no_recover": (dict(input_dim=24, encoder_dim=64, num_layers=3, reduce_layer_index=1, recover_layer_index=3, num_attention_heads=2,
                             feed_forward_expansion_factor=2, conv_expansion_factor=2, conv_kernel_size=15, half_step_residual=False), 150, (150, 83, 11)),
    "dh64_full": (dict(input_dim=16, encoder_dim=128, num_layers=3, reduce_layer_index=1, recover_layer_index=2, num_attention_heads=2,
                       feed_forward_expansion_factor=4, conv_expansion_factor=2, conv_kernel_size=31, half_step_residual=True), 300, (300, 161)),
}


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def masked_rel_mhsa(x, P, p, heads, n=None, rnd=None):
    """SO.rel_mhsa with the reference's mask: the keys >= n[b] filled with -1e9 (attention.py:90-92); a clip with n[b] = 0 gets a zero context.
    rnd: the bf16-storage restatement (encoder_y_bound): q, k, v, the context and the output rounded as the library stores them, and q+u, q+vb,
    posp and P rounded as the MFMA forward rounds them"""
    B, T, d = x.shape
    a = p + ".attention"
    r_ = rnd or (lambda t: t)
    pe = SO.rel_positional_encoding(T, d, x.dtype).repeat(B, 1, 1)
    q = r_(x @ P[a + ".query_proj.weight"].t() + P[a + ".query_proj.bias"])
    k = r_(x @ P[a + ".key_proj.weight"].t() + P[a + ".key_proj.bias"])
    v = r_(x @ P[a + ".value_proj.weight"].t() + P[a + ".value_proj.bias"])
    posp = r_(pe @ P[a + ".pos_proj.weight"].t())
    if rnd is None:
        sc = SO.rel_attention_scores(q, k, posp, P[a + ".u_bias"], P[a + ".v_bias"], heads)
    else:      # the biases added before the rounding
        dh = d // heads
        qu, qv = (r_(q.view(B, T, heads, dh) + P[a + nm].view(heads, dh)) for nm in (".u_bias", ".v_bias"))
        kh = k.view(B, T, heads, dh).permute(0, 2, 3, 1)
        sc = (torch.matmul(qu.transpose(1, 2), kh)
              + SO.relative_shift(torch.matmul(qv.transpose(1, 2), posp.reshape(B, -1, heads, dh).permute(0, 2, 3, 1)))) / math.sqrt(dh)
    if n is not None:
        nn = torch.tensor([min(max(int(t), 0), T) for t in n])
        sc = sc.masked_fill((torch.arange(T).view(1, T) >= nn.view(B, 1)).view(B, 1, 1, T), -1e9)
    attn = torch.softmax(sc, -1)
    if n is not None:
        attn = attn * (nn > 0).to(attn.dtype).view(B, 1, 1, 1)
    if rnd is not None:      # P rounded where the MFMA forward rounds it: relative to the row maximum
        mx = attn.max(-1, keepdim=True).values.clamp_min(1e-300)
        attn = r_(attn / mx) * mx
    ctx = r_(torch.matmul(attn, v.view(B, T, heads, d // heads).permute(0, 2, 1, 3)).transpose(1, 2).contiguous().view(B, T, d))
    return ctx @ P[a + ".out_proj.weight"].t() + P[a + ".out_proj.bias"]


def masked_block(x, P, p, heads, n, training, half_step_residual, rnd=None):
    f = 0.5 if half_step_residual else 1.0
    s = p + ".sequential"
    r_ = rnd or (lambda t: t)
    x = r_(SO._ln(r_(x + masked_rel_mhsa(x, P, s + ".0.module", heads, n, rnd)), P, s + ".1"))
    x = r_(SO._ln(r_(x + f * SO.feed_forward(x, P, s + ".2.module")), P, s + ".3"))
    x = r_(SO._ln(r_(x + SO.conv_module(x, P, s + ".4.module", training, None)), P, s + ".5"))
    return r_(SO._ln(r_(x + f * SO.feed_forward(x, P, s + ".6.module")), P, s + ".7"))


def masked_encoder(x, P, cfg, lengths=None, training=False, mut=(), rnd=None):
    """SO.encoder with the padding mask in every attention layer; lengths None: SO.encoder itself, restated.  Mistake: n2_in_reduced (the
    subsampled length used in the reduced layers).  rnd: see masked_rel_mhsa"""
    st = None if lengths is None else stage_lengths(lengths, x.shape[1])
    h = SO.conv2d_subsampling(x, P)
    h = h @ P["input_proj.0.weight"].t() + P["input_proj.0.bias"]
    recover_tensor, stage = None, 0
    for idx in range(cfg["num_layers"]):
        if idx == cfg["reduce_layer_index"]:
            recover_tensor = h
            h = SO.time_reduction(h, P)
            h = h @ P["time_reduction_proj.weight"].t() + P["time_reduction_proj.bias"]
            stage = 1
        if idx == cfg["recover_layer_index"]:
            h = SO.recover_resolution(h)
            length = h.shape[1]
            h = h @ P["time_recover_layer.weight"].t() + P["time_recover_layer.bias"]
            h = h + recover_tensor[:, :length, :]
            stage = 2
        wrapped = cfg["reduce_layer_index"] <= idx < cfg["recover_layer_index"]
        p = f"layers.{idx}" + (".module" if wrapped else "")
        n = None if st is None else st[0 if (stage == 1 and "n2_in_reduced" in mut) else stage]
        y = masked_block(h, P, p, cfg["num_attention_heads"], n, training, cfg.get("half_step_residual", False), rnd)
        h = y + h if wrapped else y
    return h


@functools.lru_cache(maxsize=None)
def encoder_reference(name, with_lengths=True, mut=()):
    """(x, Gm, params fp64 with .grad, y, dx) of the fp64 training pass of an encoder case; with_lengths False: the unmasked pass"""
    cfg, T0, L = ENC_CASES[name]
    B = len(L)
    P = SO.init_params(cfg, seed=5, dtype=torch.float64)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T0, cfg["input_dim"], generator=g)
    for k, v in P.items():
        v.requires_grad_(not k.endswith(("running_mean", "running_var")))
    xo = x.double().requires_grad_(True)
    yo = masked_encoder(xo, P, cfg, L if with_lengths else None, training=True, mut=mut)
    Gm = torch.randn(yo.shape, generator=g)
    (yo * Gm.double()).sum().backward()
    return x, Gm, P, yo.detach(), xo.grad


@functools.lru_cache(maxsize=None)
def encoder_y_bound(name):
    """bf16 bound of the encoder output's max-abs error: 0.1 (test_golden_squeezeformer_gpu's), or, where larger, 2 x the error of the fp64
    restatement that rounds to bf16 what it can reach of what the library stores (block inputs, q, k, v, the context, every residual sum and
    LayerNorm output) and what the MFMA forward rounds (q+u, q+vb, posp, P).  The FFN's and the convolution module's inner tensors are not
    rounded, so the restatement errs on the low side.  Computed on the CPU from the reference alone"""
    cfg, T0, lens = ENC_CASES[name]
    P = SO.init_params(cfg, seed=5, dtype=torch.float64)
    x = torch.randn(len(lens), T0, cfg["input_dim"], generator=torch.Generator().manual_seed(1)).double()
    with torch.no_grad():
        y = masked_encoder(x, P, cfg, lens, training=True)
        yr = masked_encoder(x, P, cfg, lens, training=True, rnd=_bf16)
    return max(0.1, 2.0 * float((yr - y).abs().max()))
