"""Helpers of tests/test_frame_mask.py, test_frame_mask_mutants.py and test_frame_mask_gpu.py: the three modules of the Keras hybrid that a
padding mask changes (Conv1DBlock: the ECA mean; MultiHeadSelfAttention: the keys; the Squeezeformer ConvModule: the Squeeze-Excite mean),
restated in fp64 with per-clip frame lengths from the oracle's own dense / batch_norm / causal_dwconv / layer_norm, with switchable
mistakes; the whole model chained through oracle.forward's structure; the cases and inputs the GPU test runs; per-shape bf16 bounds.

Clip b has n_b = lens[b] real frames; the mask is t < n_b.  n_b = 0: both masked means are 0 and the clip's attention output is 0 (Keras
gives NaN there).  Metrics, compare and bounds are module_parity's."""
import numpy as np
import torch

import module_parity as MP
from oracle import ishara_oracle as O

# ------------------------------------------------------------------ the GPU test's cases (shared with the CPU mutant test)
T_SMALL, B_SMALL = 72, 3
LENS = {"ragged": (72, 37, 9), "edge": (72, 0, 1)}       # T % 16 == 8: a partial last key chunk; 9: below one chunk; 0 / 1: the n_b = 0 convention
T_D512, LENS_D512 = 136, (129, 64)
SHAPES = {
    "cfg2": dict(dim=256, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, kernel_sizes=[11, 5, 3], num_conv_per_block=3, num_heads=8,
                 expansion_factor=2, transformer_kernel_size=15, input_shape=(T_SMALL, 224)),
    "d512": dict(dim=512, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, kernel_sizes=[11, 5, 3], num_conv_per_block=3, num_heads=8,
                 expansion_factor=2, transformer_kernel_size=15, input_shape=(T_D512, 224)),
}
MODULES = ["convsqueeze_0_1", "convsqueeze_0_2", "convsqueeze_0_3", "squeezeformer_0/mha", "squeezeformer_0/conv", "conformer_0/mha"]
SEED = 4242

# Per-shape bf16 bounds (module_parity.BF16_BOUND_AT's rule): 2 x the error of the fp64 restatement with bf16-rounded stored activations
# (reference(..., mut=("bf16_storage",))) against the clean one, the worst over the kind's modules and both dropout rates — measured on the
# reference alone, recomputed by test_frame_mask_mutants.test_per_shape_bounds_are_twice_the_restatement.  As in module_parity, no rel-L2
# entry exceeds BF16_CAP (there is none here: every rel-L2 holds the benchmark-shape bound); the elem entries are what they measure.
# Keyed by (kind, shape) or (kind, shape/length set).
#   conv: the implied batch statistics average bf16 rounding over B * T = 216 rows, against 768 or more at the benchmark's shapes
#         (restatement 8.7e-4).
#   mha:  the elem metric divides by the tensor's rms + |ref|.  A key that stands alone in its clip (n_b = 1) collects dk / dv from all 72
#         queries, a key of the 9-frame clip from 72 queries over 9 keys: its dqkv row is several times the tensor's rms, it is STORED IN BF16
#         (as without lengths), and the QKV dgrad spreads that rounding over every element of the row's dx, also the small ones.  Restatement:
#         dx_elem 8.9e-3 at (72, 37, 9); 4.28e-2 and y_elem 1.03e-2 (o is one bf16 value row, not a mean over keys) at (72, 0, 1).  The MI355X
#         agrees with the restatement to three digits where dropout is off (8.05e-3 / 8.05e-3, 3.18e-2 / 3.18e-2); rel-L2 stays at 2e-3.
BF16_BOUND_AT = {
    ("conv", "cfg2"): dict(stat=0.00174),
    ("mha", "cfg2/ragged"): dict(dx_elem=0.0178),
    ("mha", "cfg2/edge"): dict(dx_elem=0.0856, y_elem=0.0206),
}
assert all(v <= MP.BF16_CAP for b in BF16_BOUND_AT.values() for q, v in b.items() if q.endswith("_l2"))


def bounds(kind, dtype, shape, lens_id=None):
    b = MP.bounds(kind, dtype)
    if dtype != "bf16":
        return b
    return {**b, **BF16_BOUND_AT.get((kind, shape), {}), **BF16_BOUND_AT.get((kind, f"{shape}/{lens_id}"), {})}


def ocfg(shape, dropout):
    kw = dict(SHAPES[shape])
    kw["kernel_sizes"] = tuple(kw["kernel_sizes"])
    return O.Config(dropout_rate=dropout, head_dropout=0.4 if dropout > 0 else 0.0, conformer_attn_dropout=0.1 if dropout > 0 else 0.0, **kw)


def case_inputs(cfg, name, B, dtype, dropout):
    """(module index, first dropout site, x, dy, seed) of a module case: what test_frame_mask_gpu feeds the probe"""
    names = MP.expected_modules(cfg)
    i = names.index(name)
    first = {n: f for n, f, _ in MP.walk_sites(cfg)}[name]
    g = np.random.default_rng(2000 + i)
    x = MP.round_to(g.standard_normal((B, cfg.T, cfg.dim)), dtype)
    dy = MP.round_to(g.standard_normal((B, cfg.T, cfg.dim)), dtype)
    seed = SEED
    if MP.module_kind(name) == "conv" and dropout > 0:
        seed = MP.mixed_droppath_seed(seed, first, B, dropout)
    return i, first, x, dy, seed


# ------------------------------------------------------------------ the masked operations
def _lens(lens, T, mut):
    n = [min(max(int(v), 0), T) for v in lens]
    if "next_clip_len" in mut:          # n_{b+1} used for clip b
        n = n[1:] + n[:1]
    return n


def frame_mask(lens, T, dtype=torch.float64):
    """[B, T] of 1 (t < n_b) and 0"""
    return (torch.arange(T)[None, :] < torch.tensor([min(max(int(v), 0), T) for v in lens])[:, None]).to(dtype)


def masked_mean(x, lens, mut=()):
    """[B, C]: mean of x [B, T, C] over t < n_b, 0 at n_b = 0"""
    B, T, _ = x.shape
    n = _lens(lens, T, mut)
    if "mean_all_T" in mut:             # the mask forgotten
        return x.mean(dim=1)
    m = frame_mask(n, T, x.dtype)
    s = (x * m[:, :, None]).sum(dim=1)
    cnt = torch.tensor([float(T) if "sum_over_T" in mut else float(v) for v in n], dtype=x.dtype)      # sum_over_T: the masked sum divided by T
    mean = torch.where(cnt[:, None] > 0, s / cnt.clamp(min=1.0)[:, None], torch.zeros_like(s))
    if "gate_grad_all_T" in mut:        # the right value, its gradient spread over all T frames
        full = x.mean(dim=1)
        return mean.detach() + (full - full.detach())
    return mean


def eca_masked(x, w, lens, mut=()):
    """oracle.eca with GlobalAveragePooling1D()(x, mask=mask) (c5:8-9)"""
    g = masked_mean(x, lens, mut)
    k = w.shape[0]
    z = torch.nn.functional.conv1d(g.unsqueeze(1), w.view(1, 1, k), padding=(k - 1) // 2).squeeze(1)
    return x * torch.sigmoid(z)[:, None, :]


def _batch_norm(x, P, name, momentum, new_stats, lens, mut, training=True):
    if not training:
        return O.batch_norm(x, P, name, False, momentum, new_stats)
    if "bn_valid_only" not in mut:
        return MP._batch_norm(x, P, name, momentum, new_stats, mut)      # the oracle's arithmetic (+ bf16_storage): statistics over all B * T rows
    m = frame_mask(lens, x.shape[1], x.dtype)[:, :, None]                # the mistake: statistics over the valid frames only
    cnt = m.sum()
    mean = (x * m).sum(dim=(0, 1)) / cnt
    var = (((x - mean) ** 2) * m).sum(dim=(0, 1)) / cnt
    new_stats[f"{name}/moving_mean"] = (P[f"{name}/moving_mean"] * momentum + mean * (1 - momentum)).detach()
    new_stats[f"{name}/moving_variance"] = (P[f"{name}/moving_variance"] * momentum + var * (1 - momentum)).detach()
    return (x - mean) * torch.rsqrt(var + O.BN_EPS) * P[f"{name}/gamma"] + P[f"{name}/beta"]


def conv1d_block(x, P, name, cfg, sites, new_stats, lens, mut=(), training=True):
    """oracle.conv1d_block (c5:41-89) with the ECA mean over the valid frames; mut has bf16_storage: module_parity.conv1d_block_mut's roundings"""
    st = MP._store(mut)
    x = st(x, fwd=False)
    h = O.swish(st(O.dense(x, P, f"{name}_expand_conv")))
    h = O.causal_dwconv(h, P[f"{name}_dwconv/depthwise_kernel"])
    h = _batch_norm(h, P, f"{name}_bn", 0.95, new_stats, lens, mut, training)
    h = st(eca_masked(h, P[f"{name}_eca/kernel"], lens, mut))
    h = O.dense(h, P, f"{name}_project_conv")
    m = sites.mask(x.shape[0], 1, cfg.dropout_rate, x)
    if m is not None:
        h = h * m[:, :, None]
    return st(h + x, bwd=False)


def mhsa(x, P, name, cfg, rate, sites, lens, mut=()):
    """oracle.mhsa (c5:91-118) with the keys j >= n_b excluded for every query and head of clip b; a clip without a valid key: o = 0"""
    B, T, d = x.shape
    H = cfg.num_heads
    dh = d // H
    n = _lens(lens, T, mut)
    if "key_len_off_by_one" in mut:
        n = [min(v + 1, T) for v in n]
    st = MP._store(mut)      # bf16_storage: the normalised input, q / k / v, the probabilities as the PV operand, o and (backward) dS, dqkv, dxn are bf16 tensors
    qkv = st(O.dense(st(x), P, f"{name}/qkv", bias=False)).view(B, T, H, 3 * dh).permute(0, 2, 1, 3)
    q, k, v = qkv[..., :dh], qkv[..., dh:2 * dh], qkv[..., 2 * dh:]
    s = st((q @ k.transpose(-1, -2)) * (d ** -0.5), fwd=False)
    km = frame_mask(n, T, x.dtype)[:, None, None, :]                      # [B, 1, 1, T] over the keys
    smax = s.masked_fill(km == 0, -float("inf")).amax(dim=-1, keepdim=True)
    smax = torch.where(torch.isfinite(smax), smax, torch.zeros_like(smax)).detach()
    e = torch.exp((s - smax).masked_fill(km == 0, 0.0)) * km
    den = e.sum(dim=-1, keepdim=True)
    attn = e / torch.where(den > 0, den, torch.ones_like(den))
    m = sites.mask(B * H * T, T, rate, x, attn=True)                      # the same hash and keys as without a mask
    if m is not None:
        attn = attn * m.view(B, H, T, T)
    o = st((st(attn, bwd=False) @ v).permute(0, 2, 1, 3).reshape(B, T, d))
    return O.dense(o, P, f"{name}/proj", bias=False)


def sqz_mha(x, P, name, cfg, sites, lens, mut=()):
    r, st = cfg.dropout_rate, MP._store(mut)
    x = st(x, fwd=False)                     # (bf16_storage: the module's dx and y are bf16 tensors)
    return st(x + O._drop(mhsa(O.layer_norm(x, P, f"{name}/norm2", 1e-6), P, f"{name}/mha", cfg, r, sites, lens, mut), r, sites), bwd=False)


def conf_mha(x, P, name, cfg, sites, lens, mut=()):
    st = MP._store(mut)
    x = st(x, fwd=False)
    return st(x + mhsa(O.layer_norm(x, P, f"{name}/layer_norm1", 1e-6), P, f"{name}/mha", cfg, cfg.conformer_attn_dropout, sites, lens, mut), bwd=False)


def sqz_conv(x, P, name, cfg, sites, lens, mut=()):
    """oracle.sqz_conv (c5:135-153) with the Squeeze-Excite mean over the valid frames (c5:129-130)"""
    u = O.layer_norm(x, P, f"{name}/conv/norm", 1e-6)
    u = O.swish(O.dense(u, P, f"{name}/conv/conv1"))
    u = O.swish(O.causal_dwconv(u, P[f"{name}/conv/conv2/depthwise_kernel"]))
    u = O.dense(u, P, f"{name}/conv/conv3")
    z = masked_mean(u, lens, mut)
    z = O.swish(O.dense(z, P, f"{name}/conv/se/fc1"))
    z = torch.sigmoid(O.dense(z, P, f"{name}/conv/se/fc2"))
    return u * z[:, None, :] + x


def module_forward(name, xt, P, cfg, sites, new_stats, lens, mut=(), training=True):
    kind = MP.module_kind(name)
    if kind == "conv":
        return conv1d_block(xt, P, name, cfg, sites, new_stats, lens, mut, training)
    blk = name.split("/")[0]
    if kind == "sqzconv":
        return sqz_conv(xt, P, blk, cfg, sites, lens, mut)
    assert kind == "mha", name
    return (sqz_mha if blk.startswith("squeezeformer") else conf_mha)(xt, P, blk, cfg, sites, lens, mut)


def reference(name, cfg, W, x, dy, seed, first_site, lens, mut=()):
    """module_parity.reference for a conv / mha / sqzconv module with frame lengths: fp64 forward and autograd backward"""
    P = {}
    for k, v in W.items():
        if MP.owns(name, k):
            t = torch.from_numpy(np.asarray(v, np.float64))
            P[k] = t.requires_grad_(True) if "moving_" not in k else t
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    sites = O._Sites(seed, True, first=first_site)
    new_stats = {}
    y = module_forward(name, xt, P, cfg, sites, new_stats, lens, mut)
    y.backward(torch.from_numpy(np.asarray(dy, np.float64)))
    grads = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items() if v.requires_grad}
    return dict(y=y.detach().numpy(), dx=xt.grad.numpy().copy(), grads=grads, stats={k: v.numpy() for k, v in new_stats.items()}, loss=None,
                sites_used=sites.n - first_site)


# ------------------------------------------------------------------ the whole model
def forward(P, x, cfg, lens, training=False, seed=0):
    """oracle.forward's structure with the three masked modules; everything else is the oracle's own function"""
    sites = O._Sites(seed, training)
    new_stats = {}
    h = O.stem(x, P, cfg, training, new_stats)

    def conv_blocks(h, tag):
        for j in range(cfg.num_conv_per_block):
            h = conv1d_block(h, P, f"conv{tag}_{j + 1}", cfg, sites, new_stats, lens, training=training)
        return h

    for i in range(cfg.num_conv_squeeze_blocks):
        h = conv_blocks(h, f"squeeze_{i}")
        n = f"squeezeformer_{i}"
        h = O.sqz_ffn1(h, P, n, cfg, sites)
        h = sqz_mha(h, P, n, cfg, sites, lens)
        h = sqz_conv(h, P, n, cfg, sites, lens)
        h = O.sqz_ffn2(h, P, n, cfg, sites)
    for i in range(cfg.num_conv_conform_blocks):
        h = conv_blocks(h, f"conform_{i}")
        n = f"conformer_{i}"
        h = O.conf_ffn1(h, P, n, cfg, sites)
        h = conf_mha(h, P, n, cfg, sites, lens)
        h = O.conf_conv(h, P, n, cfg, training, new_stats)
        h = O.conf_ffn2(h, P, n, cfg, sites)
    return O.head(h, P, cfg, sites), new_stats


def loss_and_grads(params, x, y, cfg, lens, training=True, seed=0, dtype=torch.float64):
    """oracle.loss_and_grads with frame lengths: (loss, logits, grads, new_stats); the CTC loss keeps logit_length = T"""
    P = O.to_torch(params, dtype)
    xt = torch.from_numpy(np.asarray(x)).to(dtype)
    logits, new_stats = forward(P, xt, cfg, lens, training=training, seed=seed)
    loss = O.ctc_loss(torch.from_numpy(np.asarray(y)).long(), logits)
    loss.backward()
    grads = {k: v.grad.numpy() for k, v in P.items() if v.grad is not None}
    return float(loss.detach()), logits.detach().numpy(), grads, {k: v.numpy() for k, v in new_stats.items()}


def frame_lengths_np(x):
    """numpy restatement of ishara_frame_lengths: 1 + the index of the last frame with any non-zero feature, 0 if none"""
    nz = (np.asarray(x) != 0).any(axis=2)
    T = nz.shape[1]
    return np.where(nz.any(axis=1), T - np.argmax(nz[:, ::-1], axis=1), 0).astype(np.int32)
