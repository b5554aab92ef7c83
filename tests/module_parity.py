"""Helpers of tests/test_modules_gpu.py, tests/test_modules_ragged_gpu.py and tests/test_module_mutants.py: one module of the Keras hybrid (stem, Conv1DBlock, the four
sub-modules of a Squeezeformer / Conformer block, head) evaluated alone in fp64 by the oracle's own functions, the metrics both tests
compare with, and the bounds.

Metrics
  activation-shaped tensors (y, dx, the implied BatchNorm batch statistics):
    elem   max |got - ref| / (rms(ref) + |ref|): the smallest t for which |err| <= t * rms + t * |ref| holds everywhere (test_ops_gpu.close
           with atol = t * rms(ref), rtol = t)
    l2     the worst per-sample relative L2 error (one wrong sample or edge tile cannot hide in the batch)
  parameter gradients:
    l2     per-tensor relative L2 error;  max: max-abs error over the tensor's max-abs
    f32 only: elem over sqrt(rows) — |err| <= t * (sqrt(B * T) * rms + |ref|), the operator tests' bound for sums over rows

Bounds
  f32: the operator bounds of tests/test_ops_gpu.py (t = 2e-4) and test_model_gpu.py's 1e-3 of the tensor's max for gradients.
  bf16: 2x the largest value observed on the MI355X per module kind and quantity, never above BF16_CAP = 0.03 relative L2.
        BF16_BOUND_AT: per-shape entries for the short sequences of the ragged test, 2x a reference-side measurement of bf16 storage rounding.
"""
import os
import re

import numpy as np
import torch

from oracle import ishara_oracle as O
from oracle import rng

BF16_CAP = 0.03
F32_T = 2e-4          # rtol = atol of the operator tests
F32_GRAD_MAX = 1e-3   # test_model_gpu.py: gradients within 1e-3 of each tensor's max

# 2 x the largest error observed on the MI355X over every case of tests/test_modules_gpu.py (both routes, all variants), per module kind:
#   y_elem y_l2 dx_elem dx_l2 | grad_l2 grad_max (tensors of more than 8 elements) | small_l2 (the 5-tap ECA kernel: 2x observed is 0.039, held at
#   the cap) | stat (implied batch statistics, elem) | zero (a gradient that is analytically 0, over the module's largest gradient)
# `loss` (head only): relative error of the CTC loss.  No *_l2 entry exceeds BF16_CAP.  The observed values are tabulated in DESIGN.md §2.
BF16_BOUND = {
    "stem":     dict(y_elem=0.015, y_l2=0.0051, grad_l2=0.0039, grad_max=0.0048, stat=0.00085),
    "conv":     dict(y_elem=0.014, y_l2=0.0044, dx_elem=0.015, dx_l2=0.0047, grad_l2=0.019, grad_max=0.049, small_l2=0.03, stat=0.0009),
    "ffn":      dict(y_elem=0.015, y_l2=0.0043, dx_elem=0.027, dx_l2=0.005, grad_l2=0.0064, grad_max=0.0086),
    "mha":      dict(y_elem=0.0063, y_l2=0.0034, dx_elem=0.0064, dx_l2=0.0034, grad_l2=0.0082, grad_max=0.0071),
    "sqzconv":  dict(y_elem=0.0062, y_l2=0.0034, dx_elem=0.0063, dx_l2=0.0034, grad_l2=0.0087, grad_max=0.023),
    "confconv": dict(y_elem=0.043, y_l2=0.0091, dx_elem=0.024, dx_l2=0.0062, grad_l2=0.022, grad_max=0.07, stat=0.00014, zero=0.066),
    "head":     dict(y_elem=0.017, y_l2=0.0034, dx_elem=0.14, dx_l2=0.023, grad_l2=0.0043, grad_max=0.0037, loss=1.5e-05),
}
# Per-shape entries for the short sequences of tests/test_modules_ragged_gpu.py, where a quantity that AVERAGES bf16 storage rounding over the
# B * T rows has 5 to 170 times fewer rows to average over than at the benchmark's shapes.  Each is 2 x the error of the module's fp64
# restatement with its stored activations rounded to bf16 (reference(..., mut=("bf16_storage",)): z1 / h2 / h4 of a Conv1DBlock, the head's
# dropped ReLU output and the gradients it stores) against the clean fp64 reference, the worst over the kind's modules and the dropout rates
# the GPU test runs at that shape — measured on the reference alone (test_module_mutants.test_per_shape_bounds_are_twice_the_restatement
# recomputes them).  The MI355X agrees with the restatement to three digits, the f32 runs of the same shapes hold 2e-4.
#   conv t72 (144 rows): implied batch statistics, restatement 9.97e-4 / 2.20e-3 / 1.54e-3 for k = 11 / 5 / 3
#   head: CTC loss, restatement 2.31e-5 (t72), 2.97e-5 (t200, dropout 0), 3.44e-5 (t224, dropout 0); top_conv/kernel gradient at t224 with
#   dropout (dlogits stored in bf16 from M = 448 = 7 * 64 on): l2 4.42e-3, max 4.57e-3
BF16_BOUND_AT = {
    ("conv", "t72"):  dict(stat=0.0044),
    ("head", "t72"):  dict(loss=4.6e-05),
    ("head", "t200"): dict(loss=5.9e-05),
    ("head", "t224"): dict(loss=6.9e-05, grad_l2=0.0088, grad_max=0.0091),
}
assert all(v <= BF16_CAP for b in list(BF16_BOUND.values()) + list(BF16_BOUND_AT.values()) for q, v in b.items() if q.endswith("_l2"))


def bounds(kind, dtype, shape=None):
    """shape: a case label of tests/test_modules_ragged_gpu.py with entries of its own in BF16_BOUND_AT (bf16 only)"""
    if dtype == "bf16":
        return {**BF16_BOUND[kind], **BF16_BOUND_AT.get((kind, shape), {})}
    return dict(y_elem=F32_T, y_l2=F32_T, dx_elem=F32_T, dx_l2=F32_T, grad_l2=F32_GRAD_MAX, grad_max=F32_GRAD_MAX, small_l2=F32_GRAD_MAX,
                grad_elem_rows=F32_T, stat=F32_T, loss=1e-5, zero=1e-3)


# ------------------------------------------------------------------ metrics
def _err(got, ref, alts=()):
    """|got - ref| elementwise; with alternative references (a derivative the reference cannot decide: see reference(), head) the distance of
    got to the interval the references span."""
    if not alts:
        return np.abs(got - ref)
    lo, hi = ref, ref
    for a in alts:
        lo, hi = np.minimum(lo, a), np.maximum(hi, a)
    return np.maximum(0.0, np.maximum(got - hi, lo - got))


def act_metrics(got, ref, alts=()):
    """(elem, worst per-sample rel-L2) of an activation-shaped tensor [B, ...]."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = _err(got, ref, alts)
    rms = float(np.sqrt(np.mean(ref * ref))) + 1e-300
    elem = float((err / (rms + np.abs(ref))).max())
    B = ref.shape[0]
    e2 = np.sqrt((err.reshape(B, -1) ** 2).sum(1))
    r2 = np.sqrt((ref.reshape(B, -1) ** 2).sum(1)) + 1e-300
    return elem, float((e2 / r2).max())


def grad_metrics(got, ref, rows, alts=()):
    """(rel-L2, max-abs / max-abs, elem over sqrt(rows)) of a parameter gradient."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = _err(got, ref, alts)
    rms = float(np.sqrt(np.mean(ref * ref))) + 1e-300
    return (float(np.linalg.norm(err) / (np.linalg.norm(ref) + 1e-300)), float(err.max() / (np.abs(ref).max() + 1e-300)),
            float((err / (np.sqrt(rows) * rms + np.abs(ref))).max()))


def stat_metric(got_new, ref_new, old, keep):
    """elem metric of the batch statistic implied by a moving-statistics update.  The library forms new = old * keep + batch * (1 - keep) in
    fp32: three roundings of about |new| * 2^-24 each, which the division by (1 - keep) magnifies 20x / 100x — up to 4 * 2^-24 * |new| /
    (1 - keep) of the implied value is that format's noise (it dominates where the batch variance is far below the moving one) and is allowed
    on top of the bound."""
    got, ref = implied_batch_stat(got_new, old, keep), implied_batch_stat(ref_new, old, keep)
    allow = 4.0 * 2.0 ** -24 * np.maximum(np.abs(np.asarray(ref_new, np.float64)), np.abs(np.asarray(got_new, np.float64))) / (1.0 - keep)
    rms = float(np.sqrt(np.mean(ref * ref))) + 1e-300
    return float((np.maximum(0.0, np.abs(got - ref) - allow) / (rms + np.abs(ref))).max())


def implied_batch_stat(new, old, keep):
    """The batch statistic a moving-statistics update new = keep * old + (1 - keep) * batch used, in fp64 from the fp32 values."""
    return (np.asarray(new, np.float64) - keep * np.asarray(old, np.float64)) / (1.0 - keep)


# ------------------------------------------------------------------ module inventory
def module_kind(name):
    if name in ("stem", "head"):
        return name
    if "/" not in name:
        return "conv"
    blk, sub = name.split("/")
    if sub in ("ffn1", "ffn2"):
        return "ffn"
    if sub == "mha":
        return "mha"
    return "sqzconv" if blk.startswith("squeezeformer") else "confconv"


def module_param_prefixes(name):
    """Parameter-name prefixes of the entries a module owns (the Conformer's layer_norm1 serves both its ffn1 and its mha)."""
    if name == "stem":
        return ["stem_conv/", "stem_bn/"]
    if name == "head":
        return ["top_conv/", "classifier/"]
    if "/" not in name:
        return [name + "_"]
    blk, sub = name.split("/")
    if blk.startswith("squeezeformer"):
        return {"ffn1": [f"{blk}/norm1/", f"{blk}/ffn1_"], "mha": [f"{blk}/norm2/", f"{blk}/mha/"], "conv": [f"{blk}/conv/"],
                "ffn2": [f"{blk}/norm3/", f"{blk}/ffn2_"]}[sub]
    return {"ffn1": [f"{blk}/ffn1/", f"{blk}/layer_norm1/"], "mha": [f"{blk}/mha/", f"{blk}/layer_norm1/"], "conv": [f"{blk}/conv/"],
            "ffn2": [f"{blk}/ffn2/", f"{blk}/layer_norm2/"]}[sub]


def owns(name, param):
    return any(param.startswith(p) for p in module_param_prefixes(name))


def bn_of(name):
    """(BatchNorm parameter prefix, keep) of a module with a BatchNorm, else None."""
    kind = module_kind(name)
    if kind == "stem":
        return "stem_bn", 0.95
    if kind == "conv":
        return name + "_bn", 0.95
    if kind == "confconv":
        return name.split("/")[0] + "/conv/batch_norm", 0.99
    return None


def expected_modules(cfg: O.Config):
    names = ["stem"]
    for tag, n in (("squeeze", cfg.num_conv_squeeze_blocks), ("conform", cfg.num_conv_conform_blocks)):
        for i in range(n):
            names += [f"conv{tag}_{i}_{j + 1}" for j in range(cfg.num_conv_per_block)]
            blk = ("squeezeformer" if tag == "squeeze" else "conformer") + f"_{i}"
            names += [f"{blk}/{s}" for s in ("ffn1", "mha", "conv", "ffn2")]
    return names + ["head"]


def walk_sites(cfg: O.Config):
    """A counting walk of the oracle's forward: [(module name, first site id, sites drawn)] in call order, from the site counter the
    oracle itself advances (every module function of oracle/ishara_oracle.py wrapped for the duration of one tiny forward pass)."""
    small = O.Config(**{**cfg.__dict__, "input_shape": (8, 8)})
    P = O.to_torch(O.init_params(small, 0), torch.float64, requires_grad=False)
    seen, state = [], {"sites": None}
    real_sites = O._Sites

    class Sites(real_sites):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            state["sites"] = self

    def wrap(fn, namer):
        def w(*a, **k):
            n0 = state["sites"].n
            out = fn(*a, **k)
            seen.append((namer(a), n0, state["sites"].n - n0))
            return out
        return w

    saved = {}
    subs = {"stem": lambda a: "stem", "head": lambda a: "head", "conv1d_block": lambda a: a[2],
            "sqz_ffn1": lambda a: a[2] + "/ffn1", "sqz_mha": lambda a: a[2] + "/mha", "sqz_conv": lambda a: a[2] + "/conv", "sqz_ffn2": lambda a: a[2] + "/ffn2",
            "conf_ffn1": lambda a: a[2] + "/ffn1", "conf_mha": lambda a: a[2] + "/mha", "conf_conv": lambda a: a[2] + "/conv", "conf_ffn2": lambda a: a[2] + "/ffn2"}
    try:
        O._Sites = Sites
        for fn, namer in subs.items():
            saved[fn] = getattr(O, fn)
            setattr(O, fn, wrap(saved[fn], namer))
        with torch.no_grad():
            O.forward(P, torch.zeros((1,) + tuple(small.input_shape), dtype=torch.float64), small, training=True, seed=1)
    finally:
        O._Sites = real_sites
        for fn, f in saved.items():
            setattr(O, fn, f)
    return seen


# ------------------------------------------------------------------ fp64 reference of one module
class _Stored(torch.autograd.Function):
    """A tensor the library keeps in bf16: the value (fwd) and / or its gradient (bwd) rounded to bf16, everything else fp64."""
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return x.to(torch.bfloat16).to(x.dtype) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (g.to(torch.bfloat16).to(g.dtype) if ctx.bwd else g), None, None


def _store(mut):
    """mut has bf16_storage: st(x, fwd=True, bwd=True) rounds where the bf16 library stores an activation (bounds derived on the reference
    side: BF16_BOUND_AT); else the identity"""
    if "bf16_storage" in mut:
        return lambda x, fwd=True, bwd=True: _Stored.apply(x, fwd, bwd)
    return lambda x, fwd=True, bwd=True: x


def _eca(x, w, mut, kept=None):
    g = x.mean(dim=1)
    k = w.shape[0]
    if "eca_wrap" in mut:          # the 5-tap convolution wraps around the channel axis instead of zero-padding it
        p = (k - 1) // 2
        gp = torch.cat([g[:, -p:], g, g[:, :p]], dim=1)
        z = torch.nn.functional.conv1d(gp.unsqueeze(1), w.view(1, 1, k)).squeeze(1)
    else:
        z = torch.nn.functional.conv1d(g.unsqueeze(1), w.view(1, 1, k), padding=(k - 1) // 2).squeeze(1)
    gate = torch.sigmoid(z)
    if "eca_gate_const" in mut:
        gate = gate.detach()
    if "gate_other_sample" in mut:  # the first sample the drop-path keeps is gated with its neighbour's gate
        v = int(np.flatnonzero(kept)[0]) if kept is not None else 0
        idx = list(range(gate.shape[0]))
        idx[v] = (v + 1) % gate.shape[0]
        gate = gate[idx]
    return x * gate[:, None, :]


def _batch_norm(x, P, name, momentum, new_stats, mut):
    xs = x                                # (bf16_storage: the statistics come from the fp32 accumulators, the normalisation reads the stored tensor)
    x = _store(mut)(x)
    if "bn_stats_skip_tail" in mut:     # the batch statistics leave out the last partial 32-step segment (T % 32 == 0: the last 8 steps)
        T = x.shape[1]
        xs = x[:, :T - (T % 32 or 8)]
    mean = xs.mean(dim=(0, 1))
    var = ((xs - mean) ** 2).mean(dim=(0, 1))
    new_stats[f"{name}/moving_mean"] = (P[f"{name}/moving_mean"] * momentum + mean * (1 - momentum)).detach()
    new_stats[f"{name}/moving_variance"] = (P[f"{name}/moving_variance"] * momentum + var * (1 - momentum)).detach()
    if "bn_stats_const" in mut:
        mean, var = mean.detach(), var.detach()
    return (x - mean) * torch.rsqrt(var + O.BN_EPS) * P[f"{name}/gamma"] + P[f"{name}/beta"]


def _dense_tail_const(h, K, mut):
    """h @ K; wgrad_tail_rows_dropped: the last M % 64 rows of the flat [B * T] axis (M % 64 == 0: the last 16) add nothing to K's gradient"""
    if "wgrad_tail_rows_dropped" not in mut:
        return h @ K
    h2 = h.reshape(-1, h.shape[-1])
    M = h2.shape[0]
    r = M % 64 or 16
    return torch.cat([h2[:M - r] @ K, h2[M - r:] @ K.detach()]).reshape(*h.shape[:-1], K.shape[1])


def conv1d_block_mut(x, P, name, cfg, sites, new_stats, mut=()):
    """oracle.conv1d_block (training) restated with switchable mistakes; mut = () is the oracle's function (test_module_mutants checks that)."""
    st = _store(mut)                   # bf16_storage: z1, h2, h4 and the block's output (their gradients t2, t1, dx) are bf16 tensors
    x = st(x, fwd=False)
    h = O.swish(st(O.dense(x, P, f"{name}_expand_conv")))
    h = O.causal_dwconv(h, P[f"{name}_dwconv/depthwise_kernel"])
    h = _batch_norm(h, P, f"{name}_bn", 0.95, new_stats, mut)
    m = sites.mask(x.shape[0], 1, cfg.dropout_rate, x)      # (the block's only site: drawn here so that a mutation can name a kept sample)
    h = st(_eca(h, P[f"{name}_eca/kernel"], mut, None if m is None else (m[:, 0] != 0).numpy()))
    b = P[f"{name}_project_conv/bias"]
    h = _dense_tail_const(h, P[f"{name}_project_conv/kernel"], mut)
    if m is None:
        return st(h + b + x, bwd=False)
    if "droppath_by_fragment" in mut:       # every row of a 16-row fragment of the flat [B * T] axis takes the scale of the fragment's first row's sample
        B, T = x.shape[:2]
        rows = torch.arange(B * T)
        m = m[(rows // 16 * 16) // T, 0].view(B, T)
    if "bias_grad_no_droppath" in mut:      # value b * m, gradient as if the drop-path scale were 1
        bm = (b * m[:, :, None]).detach() + (b - b.detach())
    else:
        bm = b * m[:, :, None]
    return st(h * m[:, :, None] + bm + x, bwd=False)


def ffn_module_mut(x, P, ln, n1, n2, rate, sites, out_drop, mut=()):
    """x + [drop](ffn(LN(x))) restated with switchable mistakes."""
    h = O.swish(O.dense(O.layer_norm(x, P, ln, 1e-6), P, n1))
    B, T, C = h.shape
    m = sites.mask(B * T, C, rate, h)
    if m is not None:
        hm = h * m.view(B, T, C)
        h = hm.detach() + (h - h.detach()) if "ffn_mask_not_in_bwd" in mut else hm
    h = _dense_tail_const(h, P[f"{n2}/kernel"], mut) + P[f"{n2}/bias"]
    if out_drop:
        h = O._drop(h, rate, sites)
    return (x.detach() if "ln_bwd_no_residual" in mut else x) + h


def head_shifted(x, P, cfg, sites, shift=None, mut=()):
    """oracle.head; shift given: the same values, the ReLU's derivative taken as 1 where the pre-activation exceeds `shift` instead of 0.
    mut has bf16_storage: the dropped ReLU output, the gradients at the pre-activation and at x, and (M % 64 == 0, M >= 256: the padded
    classifier operands of head_bwd) the gradient at the logits are bf16 tensors; the logits themselves are fp32"""
    st = _store(mut)
    M = x.shape[0] * x.shape[1]
    z = st(O.dense(st(x, fwd=False), P, "top_conv"), fwd=False)
    h = torch.relu(z) if shift is None else torch.relu(z).detach() + (z - z.detach()) * (z.detach() > shift)
    h = st(O._drop(h, cfg.head_dropout, sites), bwd=False)
    return st(O.dense(h, P, "classifier"), fwd=False, bwd=M % 64 == 0 and M >= 256), z.detach()


def reference(name, cfg, W, x, dy, seed, first_site, labels=None, mut=()):
    """fp64 forward and backward of module `name` on weights W (name -> array), input x, output gradient dy (the head: labels, CTC loss).
    Returns dict(y, dx, grads {param: array}, stats {moving statistic: new value}, loss)."""
    kind = module_kind(name)
    P = {}
    for k, v in W.items():
        if owns(name, k):
            t = torch.from_numpy(np.asarray(v, np.float64))
            P[k] = t.requires_grad_(True) if "moving_" not in k else t
    xt = torch.from_numpy(np.asarray(x, np.float64))
    if kind != "stem":
        xt.requires_grad_(True)
    sites = O._Sites(seed, True, first=first_site)
    new_stats = {}
    if kind == "stem":
        y = O.stem(xt, P, cfg, True, new_stats)
    elif kind == "conv":
        y = conv1d_block_mut(xt, P, name, cfg, sites, new_stats, mut) if mut else O.conv1d_block(xt, P, name, cfg, True, sites, new_stats)
    elif kind == "head":
        y, z = head_shifted(xt, P, cfg, sites, mut=mut)
    else:
        blk, sub = name.split("/")
        sq = blk.startswith("squeezeformer")
        if kind == "ffn" and mut:
            if sq:
                k = sub[-1]
                y = ffn_module_mut(xt, P, f"{blk}/norm{1 if k == '1' else 3}", f"{blk}/ffn{k}_dense1", f"{blk}/ffn{k}_dense2", cfg.dropout_rate, sites, True, mut)
            else:
                k = sub[-1]
                y = ffn_module_mut(xt, P, f"{blk}/layer_norm{k}", f"{blk}/ffn{k}/dense1", f"{blk}/ffn{k}/dense2", cfg.dropout_rate, sites, False, mut)
        elif sq:
            y = {"ffn1": O.sqz_ffn1, "mha": O.sqz_mha, "conv": O.sqz_conv, "ffn2": O.sqz_ffn2}[sub](xt, P, blk, cfg, sites)
        elif sub == "conv":
            y = O.conf_conv(xt, P, blk, cfg, True, new_stats)
        else:
            y = {"ffn1": O.conf_ffn1, "mha": O.conf_mha, "ffn2": O.conf_ffn2}[sub](xt, P, blk, cfg, sites)
    loss = None
    if kind == "head":
        lt = O.ctc_loss(torch.from_numpy(np.asarray(labels)).long(), y)
        lt.backward()
        loss = float(lt.detach())
    else:
        y.backward(torch.from_numpy(np.asarray(dy, np.float64)))
    grads = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in P.items() if v.requires_grad}
    out = dict(y=y.detach().numpy(), dx=None if kind == "stem" else xt.grad.numpy().copy(), grads=grads,
               stats={k: v.numpy() for k, v in new_stats.items()}, loss=loss, sites_used=sites.n - first_site)
    if kind == "head":
        # The ReLU has no derivative at 0, and among the B * T * top_dim pre-activations some lie closer to 0 than fp32 accumulation resolves
        # (|z| < tau = 2e-5 rms(z): K <= 512 products of exactly representable operands, summed in fp32 by either side): there fp64 and the
        # kernels may take different sides, each a single whole term of dx and of the top_conv gradient.  Two more backward passes take the
        # derivative as 1 above +tau and above -tau; a compared value has to lie within the bound of the interval the three references span.
        tau = 2e-5 * float(z.pow(2).mean().sqrt())
        out["alts"] = []
        for shift in (tau, -tau):
            for v in list(P.values()) + [xt]:
                v.grad = None
            ya, _ = head_shifted(xt, P, cfg, O._Sites(seed, True, first=first_site), shift, mut)
            O.ctc_loss(torch.from_numpy(np.asarray(labels)).long(), ya).backward()
            out["alts"].append(dict(dx=xt.grad.numpy().copy(), grads={k: v.grad.numpy().copy() for k, v in P.items() if v.requires_grad}))
    return out


def compare(name, dtype, B, T, got, ref, W_old, bound):
    """All asserted quantities of one module run against its reference -> (observed {quantity: worst value}, failures [text]).
    got: dict(y, dx, grads, stats[, loss]) from the HIP run (or a mutated reference); W_old: the weights before the run."""
    obs, bad = {}, []

    def see(q, v, what):
        if v > obs.get(q, (0.0, ""))[0] or q not in obs:
            obs[q] = (v, what)
        if q in bound and not v <= bound[q]:
            bad.append(f"{what}: {q} {v:.3e} > {bound[q]:.3e}")

    e, l2 = act_metrics(got["y"], ref["y"])
    see("y_elem", e, "y"); see("y_l2", l2, "y")
    alts = ref.get("alts", ())
    if ref["dx"] is not None:
        e, l2 = act_metrics(got["dx"], ref["dx"], [a["dx"] for a in alts])
        see("dx_elem", e, "dx"); see("dx_l2", l2, "dx")
    gscale = max(float(np.abs(v).max()) for v in ref["grads"].values())
    for n, rg in ref["grads"].items():
        gg = got["grads"][n]
        if np.abs(rg).max() < 1e-6 * gscale:      # analytically zero (a conv bias in front of BatchNorm): rounding residue only, as in test_model_gpu.py
            see("zero", float(np.abs(gg).max() / gscale), n)
            continue
        l2, mx, er = grad_metrics(gg, rg, B * T, [a["grads"][n] for a in alts])
        if rg.size <= 8:
            see("small_l2", l2, n)
        else:
            see("grad_l2", l2, n); see("grad_max", mx, n)
        see("grad_elem_rows", er, n)
    bn = bn_of(name)
    if bn is not None:
        pre, keep = bn
        for leaf in ("moving_mean", "moving_variance"):
            k = f"{pre}/{leaf}"
            see("stat", stat_metric(got["stats"][k], ref["stats"][k], W_old[k], keep), k)
    if ref.get("loss") is not None:
        see("loss", abs(got["loss"] - ref["loss"]) / abs(ref["loss"]), "loss")
    return {q: v for q, (v, _) in obs.items()}, bad


def mixed_droppath_seed(seed, site, B, rate):
    """The first seed >= `seed` whose drop-path draw over B samples has a dropped and a kept sample (oracle/rng.py)."""
    for s in range(seed, seed + 4096):
        k = rng.keep_mask(s, site, B, 1, rate)[:, 0]
        if k.any() and not k.all():
            return s
    raise AssertionError("no seed with a mixed drop-path draw")


def round_to(a, dtype):
    """fp32 array rounded to the storage dtype's values."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return (t.to(torch.bfloat16).float() if dtype == "bf16" else t).numpy()


def perturbed(W, dtype):
    """test_model_gpu._perturb on a name -> array dict (non-trivial gains, biases and moving statistics); bf16: every Dense kernel rounded
    to bf16, so that the library's bf16 weight shadows are exact and weight rounding is no part of the error."""
    g = np.random.default_rng(11)
    W = dict(W)
    for n in W:
        leaf = n.rsplit("/", 1)[-1]
        if leaf in ("gamma",): W[n] = (1.0 + 0.2 * g.standard_normal(W[n].shape)).astype(np.float32)
        elif leaf in ("beta", "bias"): W[n] = (0.1 * g.standard_normal(W[n].shape)).astype(np.float32)
        elif leaf == "moving_mean": W[n] = (0.1 * g.standard_normal(W[n].shape)).astype(np.float32)
        elif leaf == "moving_variance": W[n] = (1.0 + 0.3 * g.random(W[n].shape)).astype(np.float32)
        elif dtype == "bf16" and leaf == "kernel" and W[n].ndim == 2 and "depthwise" not in n:
            W[n] = round_to(W[n], "bf16")
    return W


PROLOGUE_RE = re.compile(r"gemm_nt_as_kernel<bf16,\d+,\d+,0,([12])>|gemm_nt_as_chunk_kernel<bf16,\d+,\d+,([12])>")


def prologue_kinds(report):
    """{1 (LayerNorm), 2 (per-sample affine)} prologues of the A-stationary GEMM named in a profile report."""
    return {int(a or b) for k in report for a, b in PROLOGUE_RE.findall(k)}
