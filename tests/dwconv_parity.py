"""Helpers of tests/test_dwconv_bwd_gpu.py and tests/test_dwconv_mutants.py: the cases of the depthwise-conv backward kernels (dwconv_bwd.hip's
one-pass kernel with and without the BatchNorm backward folded in, its two weight-gradient kernels, and the forward kernels of dwconv.hip run
as data gradient), their fp64 reference, the counting inputs, the metrics and the bounds.

Reference   fp64 autograd through test_ops_gpu._dw_ref on the operands the kernel receives (x, dy rounded to the storage dtype, w f32).  With a
            BatchNorm the upstream gradient is dyc = a (dy sg + E - (h - mean) rstd Fc) in fp64.  The `consistent` cases instead derive h, mean,
            rstd, a, E = -sum(dy)/M and Fc = sum(dy xhat)/M from the conv's own fp64 output and compare dx with autograd through
            BN_batchstats(conv(f(x))): the meaning of the coefficients is then tied to BatchNorm itself (dbias is analytically 0 there and is
            not asked for; dw is compared with the formula reference).
Counting    dy = 1, x = 1, no input op, w small multiples of 1/4: dbias = B T, dw[j] = B #{t : 0 <= t - padl + j < T} and
            dx[b,t] = sum_j w[j] [0 <= t + padl - j < T] are exact in bf16 and in fp32 in any order of summation: equality, not a tolerance.
Metrics     module_parity's: dx as an activation (elem, worst per-sample relative L2), dw / dbias as parameter gradients (relative L2,
            max-abs over max-abs, elem over sqrt(rows)).  Every element counts.
Bounds      f32: the operator bounds (dx elem and l2 2e-4; dw / dbias within 1e-3 of the tensor's max and 2e-4 (sqrt(B T) rms + |ref|)).
            bf16 dw / dbias without BatchNorm: the same (fp32 arithmetic on operands that are exact in bf16).
            bf16 dx, and dw / dbias behind a BatchNorm (the transformed row is rounded to bf16 on its way into the window): BF16_BOUND, 2x the
            largest figure observed on the MI355X over all cases and routes, dx without and behind a BatchNorm kept apart, no
            relative L2 above 0.03.
"""
import zlib
from collections import namedtuple

import numpy as np
import torch

from module_parity import act_metrics, grad_metrics
from test_ops_gpu import _dw_ref

F32, BF16 = 0, 1
NONE, SWISH, GLU = 0, 1, 2
SCR, BN = 2, 4                                # flag bits of ishara_debug_dwconv_kernel_name
FORCE_LDS = 4                                 # ishara_debug_force_regstage: the LDS-tiled kernels
DW_START, DBIAS_START = 0.25, -0.5            # dw and dbias are accumulated into: what they hold before the call
BN_EPS = 1e-3

FUSED, FUSED_BN = "dwconv_bwd_fused_kernel", "dwconv_bwd_fused_kernel<BN>"
REG, TILE11, TILE15, TILE31 = "dwconv_reg_kernel", "dwconv_kernel<11,11>", "dwconv_kernel<0,15>", "dwconv_kernel<0,31>"
WIN, TILE_PART, TILE_ATOMIC = "dwconv_wgrad_win_kernel", "dwconv_wgrad_kernel<part>", "dwconv_wgrad_kernel<atomic>"

# group: what the case is there for; bias: dbias is asked for; scratch: the partial-row scratch is given; force: the LDS-tiled kernels are forced;
# bn: None | "block" (Conv1DBlock: sg given, E per sample) | "conf" (Conformer: sg NULL, E per channel); consistent: see above; kernel: the
# kernel the case is for (the GPU test asserts that the route agrees)
Case = namedtuple("Case", "group dtype inop B T C k padl bias scratch force bn consistent kernel")


def case_id(c):
    tag = "".join(["b" if c.bias else "", "" if c.scratch else "-noscr", "-lds" if c.force else "", f"-bn{c.bn}" if c.bn else "", "-auto" if c.consistent else ""])
    return f"{c.group}-{c.dtype}-op{c.inop}-B{c.B}T{c.T}C{c.C}k{c.k}p{c.padl}{tag}"


def seg_of(k):
    return 48 if k >= 11 else 32              # run_dw_fused: steps per (sample, segment) item


def tile_of(k):
    return TILE11 if k == 11 else (TILE15 if k <= 15 else TILE31)


def pad(code, k):
    return {"c": k - 1, "s": (k - 1) // 2, "0": 0}[code]


def sweep(k):
    s = seg_of(k)
    return sorted({1, k - 1, k, k + 1, s - 1, s, s + 1, 2 * s - 1, 2 * s + 1})


def _cases():
    out = []
    fused_k = {"bf16": (3, 5, 11, 15), "f32": (3, 5)}
    bn_k = {"bf16": (3, 5, 11), "f32": (3, 5)}

    def add(group, dtype, inop, B, T, C, k, padl, kernel, bias=True, scratch=True, force=False, bn=None, consistent=False):
        out.append(Case(group, dtype, inop, B, T, C, k, padl, bias, scratch, force, bn, consistent, kernel))

    # ---- the one-pass kernel
    for dt, ks in fused_k.items():
        for k in ks:
            for pc in ("c", "s") + (("0",) if k == 15 else ()):
                for i, T in enumerate(sweep(k)):
                    add("fused-T", dt, (i + k) % 3, 2, T, 128, k, pad(pc, k), FUSED)
            for inop in (NONE, SWISH, GLU):
                for bias in (True, False):
                    add("fused-op", dt, inop, 2, seg_of(k) + 1, 128, k, pad("c" if inop == SWISH else "s", k), FUSED, bias=bias)
    for dt, ks in (("bf16", (5, 11)), ("f32", (5,))):
        for k in ks:
            for i, Cc in enumerate((8, 24, 72, 256, 512, 1000, 1024)):
                add("fused-C", dt, i % 3, 2, 49, Cc, k, pad("cs"[i % 2], k), FUSED)
    for dt, ks in fused_k.items():                                               # every <K, INOP> with wave-uniform items (C/4 a multiple of 64)
        for k in ks:
            for inop in (NONE, SWISH, GLU):
                add("fused-wu", dt, inop, 2, seg_of(k) + 1, 256, k, pad("sc"[inop % 2], k), FUSED)
    add("fused-C", "bf16", SWISH, 2, 49, 1024, 15, 14, FUSED)                   # the full 64 KB of dynamic LDS
    add("fused-wrap", "bf16", SWISH, 260, 64, 1024, 3, 2, FUSED)                # 520 items on 512 workgroups
    add("fused-samples", "bf16", GLU, 3, 33, 8, 3, 1, FUSED)                    # 128 lanes over 6 items
    add("fused-samples", "f32", SWISH, 3, 33, 8, 3, 2, FUSED)
    # ---- the one-pass kernel with the BatchNorm backward
    for dt, ks in bn_k.items():
        for k in ks:
            s = seg_of(k)
            for T in sorted({1, k, s - 1, s + 1, 2 * s + 1}):
                add("bn-T", dt, SWISH, 3, T, 128, k, k - 1, FUSED_BN, bias=False, bn="block")
                add("bn-T", dt, GLU, 2, T, 128, k, (k - 1) // 2, FUSED_BN, bn="conf")
    for dt, ks in (("bf16", (5, 11)), ("f32", (5,))):
        for k in ks:
            for Cc in (24, 256, 1024):
                add("bn-C", dt, SWISH, 3, seg_of(k) + 1, Cc, k, k - 1, FUSED_BN, bias=False, bn="block")
                add("bn-C", dt, GLU, 2, seg_of(k) + 1, Cc, k, (k - 1) // 2, FUSED_BN, bn="conf")
    for dt, ks in bn_k.items():                                                  # every <K, INOP, WU> with the BatchNorm backward
        for k in ks:
            for inop in (NONE, SWISH, GLU):
                for Cc in (128, 256):
                    add("bn-var", dt, inop, 3, seg_of(k) + 1, Cc, k, pad("sc"[inop % 2], k), FUSED_BN, bias=inop != SWISH, bn="block" if inop == SWISH else "conf")
    for dt, k in (("bf16", 11), ("f32", 5)):
        add("bn-auto", dt, SWISH, 3, seg_of(k) + 1, 128, k, k - 1, FUSED_BN, bias=False, bn="conf", consistent=True)
        add("bn-auto", dt, GLU, 2, seg_of(k) + 1, 128, k, (k - 1) // 2, FUSED_BN, bias=False, bn="conf", consistent=True)
    add("bn-k15", "bf16", SWISH, 3, 49, 128, 15, 14, FUSED, bias=False, bn="block")      # not folded: the entry point answers 0
    add("bn-k15", "bf16", GLU, 2, 49, 128, 15, 7, FUSED, bn="conf")
    # ---- two passes: the register-window forward kernel as data gradient + atomic weight gradient (no scratch)
    for dt in ("f32", "bf16"):
        for k in (3, 5):
            for Cc in (8, 256, 1024):
                for T in (31, 32, 33, 129):
                    for inop in (NONE, SWISH, GLU):
                        add("reg-atomic", dt, inop, 2, T, Cc, k, pad("c" if inop == SWISH else "s", k), REG + "+" + TILE_ATOMIC, scratch=False)
    # ---- the tile kernel + the windowed weight gradient
    for k in (11, 15):
        for Cc in (72, 128, 200):
            for i, T in enumerate((1, 31, 32, 33, 63, 64, 65)):
                for pc in ("c", "s"):
                    add("tile-win", "f32", (i + Cc // 8) % 3, 2, T, Cc, k, pad(pc, k), tile_of(k) + "+" + WIN)
    add("tile-win", "bf16", SWISH, 2, 40, 1152, 11, 10, TILE11 + "+" + WIN)     # bf16 reaches it only past the one-pass kernel's C <= 1024
    # ---- the tile kernel + the tap-lane weight gradient with partial rows
    for dt in ("f32", "bf16"):
        for k in (1, 2, 7, 31):
            for Cc in (8, 200, 256):
                for i, T in enumerate((7, 32, 33, 65)):
                    add("tile-part", dt, (i + k) % 3, 2, T, Cc, k, pad("0" if k == 1 else "cs"[i % 2], k), tile_of(k) + "+" + TILE_PART)
    add("tile-part", "bf16", SWISH, 5, 450, 1024, 7, 6, TILE15 + "+" + TILE_PART)       # 75 items on 64 splits: the next item's loads in flight
    # ---- forced LDS-tiled kernels
    for dt in ("f32", "bf16"):
        for T in (33, 65):
            for k in (5, 15):
                add("forced", dt, GLU if k == 5 else SWISH, 2, T, 128, k, pad("s" if k == 5 else "c", k), tile_of(k) + "+" + TILE_ATOMIC, force=True)
    assert len(set(out)) == len(out)
    return out


CASES = _cases()


def expected_kernel(lib, c):
    """the kernel the route picks for the case's call, from the library (host only; nothing is launched)"""
    lib.ishara_debug_force_regstage(FORCE_LDS if c.force else 0)
    try:
        return lib.ishara_debug_dwconv_kernel_name(BF16 if c.dtype == "bf16" else F32, 1, c.B, c.T, c.C, c.k, c.padl, (SCR if c.scratch else 0) | (BN if c.bn else 0)).decode()
    finally:
        lib.ishara_debug_force_regstage(0)


def is_atomic(c):
    return c.kernel.endswith(TILE_ATOMIC)


def fused_variant(c):
    """<K, INOP, WU, BN> of dwconv_bwd_fused_kernel the case instantiates (None: another kernel)"""
    if not c.kernel.startswith(FUSED):
        return None
    return (c.k, c.inop, (c.C // 4) % 64 == 0, c.kernel == FUSED_BN)


# ------------------------------------------------------------------ bounds
F32_T, F32_GRAD_MAX, BF16_CAP = 2e-4, 1e-3, 0.03
# 2 x the largest figure observed on the MI355X over every bf16 case and route, per tensor, without and behind a BatchNorm (bn_*: the
# transformed row is rounded to bf16 before k taps multiply it, so dx carries k row roundings on top of its own).  Observed: dx 3.43e-3 / 2.28e-3
# (elem / l2), bn dx 2.03e-2 / 2.84e-3, bn dw 1.89e-3 / 3.01e-3 (l2 / max), bn dbias 1.81e-3 / 2.33e-3
BF16_BOUND = dict(dx_elem=0.0069, dx_l2=0.0046, bn_dx_elem=0.041, bn_dx_l2=0.0057, bn_dw_l2=0.0038, bn_dw_max=0.0061, bn_dbias_l2=0.0037, bn_dbias_max=0.0047)
assert all(v <= BF16_CAP for q, v in BF16_BOUND.items() if q.endswith("_l2"))


def bounds(c):
    """quantity -> bound"""
    exact = dict(dw_max=F32_GRAD_MAX, dw_rows=F32_T, dbias_max=F32_GRAD_MAX, dbias_rows=F32_T)
    if c.dtype == "f32":
        return dict(dx_elem=F32_T, dx_l2=F32_T, **exact)
    if not c.bn:
        return dict(dx_elem=BF16_BOUND["dx_elem"], dx_l2=BF16_BOUND["dx_l2"], **exact)
    return {q: BF16_BOUND["bn_" + q] for q in ("dx_elem", "dx_l2", "dw_l2", "dw_max", "dbias_l2", "dbias_max")}


def observe(c, got, ref):
    """quantity -> observed figure; got / ref: dict of dx [B,T,Cin], dw [k,C] and (asked for) dbias [C] as fp64 arrays, dw / dbias without
    their start values"""
    obs = {}
    obs["dx_elem"], obs["dx_l2"] = act_metrics(got["dx"], ref["dx"])
    for n in ("dw", "dbias"):
        if n in ref:
            obs[n + "_l2"], obs[n + "_max"], obs[n + "_rows"] = grad_metrics(got[n], ref[n], c.B * c.T)
    return obs


def excess(obs, bound):
    """the quantities over their bound"""
    return {q: (obs[q], b) for q, b in bound.items() if q in obs and not obs[q] <= b}


# ------------------------------------------------------------------ inputs
def _round(a, dtype):
    t = torch.as_tensor(np.asarray(a, np.float64))
    return (t.to(torch.bfloat16) if dtype == "bf16" else t.to(torch.float32)).double().numpy()


def _act(x, inop, C):
    x = torch.as_tensor(x)
    if inop == SWISH:
        return x * torch.sigmoid(x)
    if inop == GLU:
        return x[..., :C] * torch.sigmoid(x[..., C:])
    return x


def inputs(c):
    """the operands of the case as fp64 arrays holding values of the dtypes the kernel receives: x [B,T,Cin], dy [B,T,C] (storage dtype), w
    [k,C], conv bias [C] (f32) and, with a BatchNorm, h [B,T,C] (storage), mean, rstd, a, Fc [C], E [B,C] / [C], sg [B,C] / None (f32)"""
    g = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()))
    B, T, Cc, k = c.B, c.T, c.C, c.k
    Cin = 2 * Cc if c.inop == GLU else Cc
    f32 = lambda a: np.asarray(a, np.float32).astype(np.float64)
    op = dict(x=_round(g.standard_normal((B, T, Cin)), c.dtype), dy=_round(g.standard_normal((B, T, Cc)), c.dtype),
              w=f32(g.standard_normal((k, Cc)) / k ** 0.5), bias=f32(0.3 * g.standard_normal(Cc)))
    if not c.bn:
        return op
    with torch.no_grad():
        h64 = _dw_ref(torch.as_tensor(op["x"]), torch.as_tensor(op["w"]), torch.as_tensor(op["bias"]), c.inop, c.padl, Cc).numpy()
    M = B * T
    if c.consistent:
        mean, var = h64.mean((0, 1)), h64.var((0, 1))
        rstd = 1.0 / np.sqrt(var + BN_EPS)
        gamma = 1.0 + 0.2 * g.standard_normal(Cc)
        xhat = (h64 - mean) * rstd
        op.update(h=_round(h64, c.dtype), mean=f32(mean), rstd=f32(rstd), a=f32(gamma * rstd), gamma=gamma, E=f32(-op["dy"].sum((0, 1)) / M),
                  Fc=f32((op["dy"] * xhat).sum((0, 1)) / M), sg=None)
        return op
    mean = h64.mean((0, 1)) + 0.1 * g.standard_normal(Cc)
    rstd = (1.0 + 0.1 * g.uniform(-1, 1, Cc)) / np.sqrt(h64.var((0, 1)) + 0.05)
    per = c.bn == "block"
    op.update(h=_round(h64, c.dtype), mean=f32(mean), rstd=f32(rstd), a=f32((1.0 + 0.2 * g.standard_normal(Cc)) * rstd), Fc=f32(0.1 * g.standard_normal(Cc)),
              E=f32(0.1 * g.standard_normal((B, Cc) if per else Cc)), sg=f32(1.0 / (1.0 + np.exp(-g.standard_normal((B, Cc))))) if per else None)
    return op


def bn_apply(op, mut=()):
    """dyc [B,T,C] = a (dy sg + E - (h - mean) rstd Fc) in fp64"""
    E = op["E"]
    if E.ndim == 2:
        E = (E[:1] if "bn_E0" in mut else E)[:, None, :]
    sg = 1.0 if op["sg"] is None else op["sg"][:, None, :]
    Fc = 0.0 if "bn_no_Fc" in mut else op["Fc"]
    return op["a"] * (op["dy"] * sg + E - (op["h"] - op["mean"]) * op["rstd"] * Fc)


def reference(c, op=None):
    """dx, dw and (asked for) dbias in fp64 under autograd"""
    op = op or inputs(c)
    x = torch.tensor(op["x"], requires_grad=True)
    w = torch.tensor(op["w"], requires_grad=True)
    b = torch.tensor(op["bias"], requires_grad=True)
    y = _dw_ref(x, w, b, c.inop, c.padl, c.C)
    y.backward(torch.as_tensor(bn_apply(op) if c.bn else op["dy"]))
    ref = dict(dx=x.grad.numpy(), dw=w.grad.numpy())
    if c.bias:
        ref["dbias"] = b.grad.numpy()
    if c.consistent:
        x2 = torch.tensor(op["x"], requires_grad=True)
        h = _dw_ref(x2, torch.as_tensor(op["w"]), torch.as_tensor(op["bias"]), c.inop, c.padl, c.C)
        mean, var = h.mean((0, 1)), h.var((0, 1), unbiased=False)
        out = torch.as_tensor(op["gamma"]) * (h - mean) / torch.sqrt(var + BN_EPS)
        out.backward(torch.as_tensor(op["dy"]))
        ref["dx"] = x2.grad.numpy()
    return ref


# ------------------------------------------------------------------ counting inputs
def counting_inputs(c):
    """dy = 1, x = 1, no input op, taps that are multiples of 1/4 in [-1/2, 1/2]: every sum is exact in bf16 and fp32.  With a BatchNorm the
    coefficients are the identity (a = 1, E = Fc = 0, no sg) on an arbitrary h: a (dy + 0 - (h - mean) rstd 0) = dy exactly."""
    g = np.random.default_rng(zlib.crc32(repr(tuple(c)).encode()) ^ 0x5A5A)
    op = dict(x=np.ones((c.B, c.T, c.C)), dy=np.ones((c.B, c.T, c.C)), w=g.integers(-2, 3, (c.k, c.C)) / 4.0, bias=np.zeros(c.C))
    if c.bn:
        op.update(h=_round(g.standard_normal((c.B, c.T, c.C)), c.dtype), mean=np.asarray(g.standard_normal(c.C), np.float32).astype(np.float64),
                  rstd=np.ones(c.C), a=np.ones(c.C), Fc=np.zeros(c.C), E=np.zeros((c.B, c.C) if c.bn == "block" else c.C), sg=None)
    return op


def counting_expect(c, w):
    """dx [B,T,C], dw [k,C], dbias [C] of the counting inputs, as integers (dx: multiples of 1/4)"""
    t, j = np.arange(c.T)[:, None], np.arange(c.k)[None, :]
    src = t + c.padl - j                                   # the dy row tap j of step t reads
    dx = ((src >= 0) & (src < c.T)).astype(np.float64) @ w                         # [T, C]
    tin = t - c.padl + j                                   # the x row tap j meets at output step t
    cnt = ((tin >= 0) & (tin < c.T)).sum(0).astype(np.float64) * c.B                # [k]
    return dict(dx=np.broadcast_to(dx, (c.B, c.T, c.C)), dw=np.broadcast_to(cnt[:, None], (c.k, c.C)), dbias=np.full(c.C, float(c.B * c.T)))


# ------------------------------------------------------------------ the one-pass arrangement restated (tests/test_dwconv_mutants.py)
MUTANTS = ("halo_zero", "halo_prev_sample", "dbias_drop_head", "seam_twice", "dw_tail", "no_flip", "same_padl", "swish_sigma_only", "glu_no_1ms",
           "bn_E0", "bn_no_Fc", "bn_leak", "dw_overwrite")


def restate(c, op=None, mut=(), ideal_bf16=False, start=(DW_START, DBIAS_START), inop=None):
    """The one-pass kernel's arrangement in fp64: (sample, segment) items of seg_of(k) steps, a window of k rows of (BatchNorm-transformed) dy
    whose k - 1 halo rows are preloaded, the newest row entering at every step, dbias as "every row exactly once" (the rows [0, padl) of a
    sample with the preload of its first segment, every other row as it enters as the newest one), dw and dbias accumulated onto `start`.
    mut: one of MUTANTS switched on.  ideal_bf16: the BatchNorm-transformed row and dx are rounded to bf16 once, every sum stays exact.
    Returns dx, dw, dbias with the start values included."""
    op = op or inputs(c)
    inop = c.inop if inop is None else inop
    B, T, Cc, k, seg = c.B, c.T, c.C, c.k, seg_of(c.k)
    padl = (k - 1) // 2 if "same_padl" in mut else c.padl
    x, w = op["x"], op["w"]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))
    if inop == SWISH:
        s = sig(x)
        f, fp, fg = x * s, (s if "swish_sigma_only" in mut else s * (1.0 + x * (1.0 - s))), None
    elif inop == GLU:
        a_, s = x[..., :Cc], sig(x[..., Cc:])
        f, fp, fg = a_ * s, s, (a_ * s if "glu_no_1ms" in mut else a_ * s * (1.0 - s))
    else:
        f, fp, fg = x, np.ones_like(x), None
    rnd = (lambda v: _round(v, "bf16")) if ideal_bf16 else (lambda v: v)
    if c.bn:
        rows = rnd(bn_apply(op, mut))
        # what the transform makes of an out-of-range (zero) dy row with h = 0: k0 = a E + mean a rstd Fc
        E = op["E"] if op["E"].ndim == 2 else np.broadcast_to(op["E"], (B, Cc))
        leak = rnd(op["a"] * E + op["mean"] * op["a"] * op["rstd"] * op["Fc"]) if "bn_leak" in mut else np.zeros((B, Cc))
    else:
        rows, leak = op["dy"], np.zeros((B, Cc))
    dx = np.zeros_like(x)
    dw, db = np.zeros((k, Cc)), np.zeros(Cc)
    wt = w[::-1] if "no_flip" in mut else w
    for b in range(B):
        for t0 in range(0, T, seg):
            tend = min(T, t0 + seg)
            win = {}                                                       # dy row index -> the row the window holds for it
            for m in range(1, k):                                          # preload
                tin = t0 + padl - k + m
                ok = 0 <= tin < T
                win[tin] = rows[b, tin] if ok else np.zeros(Cc)
                if "halo_zero" in mut and t0 > 0:
                    win[tin] = np.zeros(Cc)
                if "halo_prev_sample" in mut and t0 == 0 and tin < 0 and b > 0 and T + tin >= 0:
                    win[tin] = rows[b - 1, T + tin]
                if t0 == 0 and 0 <= tin < padl and "dbias_drop_head" not in mut:
                    db += win[tin]
            for t in range(t0, tend):
                tn = t + padl                                              # the newest row
                win[tn] = rows[b, tn] if tn < T else leak[b]
                db += win[tn]
                if "seam_twice" in mut and t == tend - 1 and tend < T:      # the last newest row of a segment is the first of the next one as well
                    db += win[tn]
                pre = np.zeros(Cc)
                for j in range(k):
                    pre += wt[j] * win[tn - j]
                    if not ("dw_tail" in mut and t >= (T // seg) * seg):
                        dw[j] += f[b, t] * win[tn - j]
                dx[b, t, :Cc] = fp[b, t, :Cc] * pre
                if fg is not None:
                    dx[b, t, Cc:] = fg[b, t] * pre
    s_dw, s_db = (0.0, 0.0) if "dw_overwrite" in mut else start
    return dict(dx=rnd(dx), dw=dw + s_dw, dbias=db + s_db)
