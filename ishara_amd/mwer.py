"""Minimum-risk (MWER) training over the beam's n-best list: the host definition and the device entries of `ishara_ctc_nbest_grad`
(csrc/ctc_nbest_grad.hip), `ishara_mwer_weights` (csrc/mwer_weights.hip) and `ishara_loss_backward_nbest` (csrc/keras_hybrid.hip); contracts
in include/ishara_hip.h.

The training side minimised only the CTC likelihood of the reference string, while every score this project reports is a normalised edit
distance.  Minimum word / character error rate training (Prabhavalkar et al. 2018, Shannon 2017) minimises the EXPECTED edit distance over
the model's own n-best list, interpolated with CTC:

  search    the n-best list of the prefix beam search, no LM; treated as a constant
  score     logp_n = log P(h_n | x), the exact CTC forward sum of every hypothesis (ishara_ctc_score_nbest)
  weights   p_n = softmax over the live slots of logp_n / temperature; W_n = edit distance of h_n to the target (divided by the target's
            length with normalise); risk = sum_n p_n W_n; coef_n = d risk / d nll_n = -p_n (W_n - risk) / temperature
  gradient  d risk / d logits = sum_n coef_n (softmax - post_n), post_n the CTC class posterior of h_n: one ishara_ctc_nbest_grad call

  ctc_posterior_reference, nbest_grad_reference, mwer_reference   one clip in numpy fp64
  ctc_nbest_grad, mwer_weights                                    device tensors in, device tensors out, on the current stream, nothing waits
  mwer_loss                                                       a torch.autograd.Function for the torch families
  Optimizer(mwer_nbest=...) / Model.mwer_stats                    the Keras-hybrid family's training step (model.py)

The reference string is not added to the list, the search uses no LM, duplicates are not merged (the prefix beam search emits distinct
prefixes).  No accuracy effect is measured anywhere in this repository: there is no dataset, there are no trained weights, and no
TensorFlow / torch MWER implementation to compare with.
"""
from __future__ import annotations

import ctypes as C_
from typing import Optional, Sequence

import numpy as np

from .rescore import MAX_CLASSES, MAX_FRAMES, MAX_HYP_LEN, MAX_NBEST, MAX_TARGET_LEN, STATUS_LONG, target_symbols

OPTION_NAMES = ("mwer_nbest", "mwer_beam_width", "mwer_weight", "mwer_ctc_weight", "mwer_temperature", "mwer_normalise", "mwer_start_step")


# ---------------------------------------------------------------------------------------------------- host references
def _log_softmax(x):
    m = x.max(axis=1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))


def ctc_posterior_reference(logits, hyp: Sequence[int], blank: int):
    """(logp, post [T, C]) of one hypothesis on one clip in fp64 by the alpha / beta recursions: post[t, k] = sum over the lattice states s
    that carry class k of exp(alpha_t[s] + beta_t[s] - lp[t, ext[s]] - logp), so d logp / d logits = post - softmax.  logits [T, C];
    logp = -inf and post = 0 when no alignment exists."""
    x = np.asarray(logits, np.float64)
    T, Cn = x.shape
    h = [int(v) for v in hyp]
    if any(v < 0 or v >= Cn or v == blank for v in h):
        raise ValueError(f"hypothesis symbols must lie in [0, {Cn}) and differ from the blank {blank}")
    lp = _log_softmax(x)
    ext = np.full(2 * len(h) + 1, blank, np.int64)
    ext[1::2] = h
    S = ext.shape[0]
    skip = np.zeros(S, bool)                                 # s-2 -> s
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    ninf = -np.inf
    al = np.full((T, S), ninf)
    be = np.full((T, S), ninf)
    al[0, 0] = lp[0, blank]
    if S > 1:
        al[0, 1] = lp[0, ext[1]]
    be[T - 1, S - 1] = lp[T - 1, blank]
    if S > 1:
        be[T - 1, S - 2] = lp[T - 1, ext[S - 2]]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a = al[t - 1]
            a1 = np.concatenate([[ninf], a[:-1]])
            a2 = np.where(skip, np.concatenate([[ninf, ninf], a[:-2]])[:S], ninf)
            al[t] =np.logaddexp(np.logaddexp(a, a1), a2) + lp[t, ext]
        for t in range(T - 2, -1, -1):
            b = be[t + 1]
            b1 = np.concatenate([b[1:], [ninf]])
            b2 = np.concatenate([np.where(skip[2:], b[2:], ninf), [ninf, ninf]])[:S]
            be[t] = np.logaddexp(np.logaddexp(b, b1), b2) + lp[t, ext]
        logp = float(np.logaddexp(al[T - 1, S - 1], al[T - 1, S - 2]) if S > 1 else al[T - 1, 0])
    post = np.zeros((T, Cn))
    if np.isfinite(logp):
        with np.errstate(invalid="ignore"):
            g = np.exp(al + be - lp[:, ext] - logp)
        g = np.where(np.isfinite(g), g, 0.0)
        for s in range(S):
            post[:, ext[s]] += g[:, s]
    return logp, post


def nbest_grad_reference(logits, hyps, coef, blank: int, grad_scale: float = 1.0):
    """One clip in fp64: (G [T, C], bound_terms [T, C], logp [N]).  G = grad_scale * sum_n coef_n (softmax - post_n) over the hypotheses
    that take part (not None, coef_n != 0, an alignment exists); bound_terms = sum_n |coef_n| |softmax - post_n|, what the per-term bound
    of tests/mwer_parity.py scales; logp_n = -inf for a slot that takes no part in the lattice sense."""
    x = np.asarray(logits, np.float64)
    sm = np.exp(_log_softmax(x))
    G = np.zeros_like(x)
    A = np.zeros_like(x)
    logp = np.full(len(hyps), -np.inf)
    for n, h in enumerate(hyps):
        if h is None:
            continue
        logp[n], post = ctc_posterior_reference(x, h, blank)
        if not np.isfinite(logp[n]) or float(coef[n]) == 0.0:
            continue
        G += float(coef[n]) * (sm - post)
        A += abs(float(coef[n])) * np.abs(sm - post)
    return grad_scale * G, A, logp


def levenshtein(a, b) -> int:
    from .evaluation import levenshtein as lev
    return int(lev([int(v) for v in a], [int(v) for v in b]))


def risk_reference(logp, dist, tlen: int, inv_temp: float, normalise: bool):
    """(W, post, risk, coef) in fp64 from the exact scores logp [N] (-inf or NaN: not live) and the distances dist [N]"""
    logp = np.asarray(logp, np.float64)
    live = np.isfinite(logp)
    W = np.asarray(dist, np.float64) / (max(int(tlen), 1) if normalise else 1)
    post = np.zeros(len(logp))
    if not live.any():
        return W, post, float("nan"), np.zeros(len(logp))
    e = np.exp((logp[live] - logp[live].max()) * float(inv_temp))
    post[live] = e / e.sum()
    risk = float((post[live] * W[live]).sum())
    coef = np.where(live, -float(inv_temp) * post * (np.where(live, W, 0.0) - risk), 0.0)
    return W, post, risk, coef


def mwer_reference(logits, hyps, target, blank: int, inv_temp: float = 1.0, normalise: bool = True) -> dict:
    """The definition in numpy fp64, one clip: logits [T, C]; hyps: N entries, each a sequence of classes or None for a dead slot; target:
    the clip's symbols (a pad-59 row is cut at the first 59).  A slot is live iff it is not None and has an alignment.
    Returns dict(logp [N], dist [N] (-1 when not live), post [N], risk, coef [N] = d risk / d nll_n, grad [T, C] = d risk / d logits by the
    analytic alpha / beta posteriors, tlen)."""
    x = np.asarray(logits, np.float64)
    tgt = target_symbols(target)
    N = len(hyps)
    logp = np.full(N, -np.inf)
    posts = [None] * N
    for n, h in enumerate(hyps):
        if h is not None:
            logp[n], posts[n] = ctc_posterior_reference(x, h, blank)
    live = np.isfinite(logp)
    dist = np.array([levenshtein(h, tgt) if lv else -1 for h, lv in zip(hyps, live)], np.int64)
    _, post, risk, coef = risk_reference(logp, dist, len(tgt), inv_temp, normalise)
    sm = np.exp(_log_softmax(x))
    grad = np.zeros_like(x)
    for n in range(N):
        if live[n]:
            grad += coef[n] * (sm - posts[n])
    return dict(logp=logp, dist=dist, post=post, risk=risk, coef=coef, grad=grad, tlen=len(tgt))


def risk_of(logits, hyps, target, blank: int, inv_temp: float = 1.0, normalise: bool = True) -> float:
    """the fp64 risk alone, by the forward algorithm only (tests difference it)"""
    from .rescore import ctc_logp_reference
    x = np.asarray(logits, np.float64)
    tgt = target_symbols(target)
    logp = np.array([-np.inf if h is None else ctc_logp_reference(x, h, blank) for h in hyps])
    dist = [levenshtein(h, tgt) if h is not None else -1 for h in hyps]
    return risk_reference(logp, dist, len(tgt), inv_temp, normalise)[2]


# ---------------------------------------------------------------------------------------------------- options of the training step
def check_options(mwer_nbest=0, mwer_beam_width=8, mwer_weight=1.0, mwer_ctc_weight=0.01, mwer_temperature=1.0, mwer_normalise=True,
                  mwer_start_step=0) -> dict:
    """The seven Optimizer(mwer_*) options, validated; returns them as a plain dict (the optional key of save_state)."""
    import math
    from .ctc_beam import MAX_BEAM

    def integer(v, what, lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
            raise ValueError(f"{what} must be an integer in {lo}..{hi}, got {v!r}")
        return int(v)

    def number(v, what, positive=False):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) or float(v) < 0 or (
                positive and float(v) == 0):
            raise ValueError(f"{what} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
        return float(v)

    nb = integer(mwer_nbest, "mwer_nbest", 0, MAX_NBEST)
    bw = integer(mwer_beam_width, "mwer_beam_width", 1, MAX_BEAM)
    if nb > bw:
        raise ValueError(f"mwer_nbest {nb} exceeds mwer_beam_width {bw}: the search keeps at most beam_width hypotheses")
    if not isinstance(mwer_normalise, (bool, np.bool_)):
        raise ValueError(f"mwer_normalise must be True or False, got {mwer_normalise!r}")
    return dict(mwer_nbest=nb, mwer_beam_width=bw, mwer_weight=number(mwer_weight, "mwer_weight"),
                mwer_ctc_weight=number(mwer_ctc_weight, "mwer_ctc_weight"),
                mwer_temperature=number(mwer_temperature, "mwer_temperature", positive=True), mwer_normalise=bool(mwer_normalise),
                mwer_start_step=integer(mwer_start_step, "mwer_start_step", 0, 2 ** 31 - 1))


# ---------------------------------------------------------------------------------------------------- device side
def workspace_bytes(lib, B: int, T: int, N: int, max_len: int) -> int:
    n = int(lib.ishara_ctc_nbest_grad_workspace_bytes(B, T, N, max_len))
    if n < 0:
        raise ValueError(f"ishara_ctc_nbest_grad takes no B={B}, T={T}, N={N}, max_len={max_len}")
    return max(n, 16)


def ctc_nbest_grad(logits, hyp_idx, hyp_len, coef, lengths=None, grad_scale: float = 1.0, out=None, accumulate: bool = False,
                   max_len: Optional[int] = None, return_logp: bool = False, blank: Optional[int] = None, dlb=None, workspace=None):
    """grad_scale * sum_n coef[b, n] * d nll_n / d logits on the device (ishara_ctc_nbest_grad).  logits fp32 [B, T, C]; hyp_idx int32
    [B, N, Th] / hyp_len int32 [B, N] as the beam search writes them; coef fp32 [B, N] (mwer_weights'); lengths: the clips' frame counts
    (None: T each); out: the fp32 [B, T, C] tensor to write (None: a new one; with accumulate the sum out + G is written, rows past a clip's
    end stay); max_len: the longest hypothesis that takes part, 1..255 (None: min(Th, 255)); it sizes the workspace, a longer slot gets
    status 8 and contributes nothing; blank defaults to C - 1; dlb: an int32 [B * T, 64] tensor for the padded bf16 copy, or None.
    Runs on the current stream, nothing waits.  Returns the gradient tensor; with return_logp (G, logp fp32 [B, N], status int32 [B, N])."""
    import torch
    from . import _lib, ctc
    from .rescore import _cuda, _nbest
    hyp_idx, hyp_len, B, N, Th = _nbest(hyp_idx, hyp_len)
    x = _cuda(logits, torch.float32, None, "logits")
    if x.ndim != 3 or x.shape[0] != B:
        raise ValueError(f"logits must be [B={B}, T, C], got {tuple(x.shape)}")
    _, T, Cn = x.shape
    if not 2 <= Cn <= MAX_CLASSES:
        raise ValueError(f"C={Cn} outside 2..{MAX_CLASSES}")
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"T={T} outside 1..{MAX_FRAMES}")
    blank = Cn - 1 if blank is None else int(blank)
    if not 0 <= blank < Cn:
        raise ValueError(f"blank {blank} outside 0..{Cn - 1}")
    max_len = min(Th, MAX_HYP_LEN) if max_len is None else int(max_len)
    if not 1 <= max_len <= MAX_HYP_LEN:
        raise ValueError(f"max_len {max_len} outside 1..{MAX_HYP_LEN}")
    coef = _cuda(coef, torch.float32, (B, N), "coef")
    if accumulate and out is None:
        raise ValueError("accumulate adds into out=: give the tensor")
    if out is None:
        out = torch.empty((B, T, Cn), dtype=torch.float32, device=x.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, T, Cn) and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous fp32 [{B}, {T}, {Cn}] tensor on the GPU")
    if dlb is not None:
        dlb = _cuda(dlb, torch.int32, (B * T, 64), "dlb")
    for t, what in ((coef, "coef"), (out, "out"), (hyp_idx, "hyp_idx"), (dlb, "dlb")):
        if t is not None and t.device != x.device:
            raise ValueError(f"logits and {what} must be on one device")
    fl = None if lengths is None else ctc._lengths(lengths, B, T, 1, "lengths", x.device)
    logp = torch.empty((B, N), dtype=torch.float32, device=x.device) if return_logp else None
    status = torch.empty((B, N), dtype=torch.int32, device=x.device) if return_logp else None
    with torch.cuda.device(x.device):
        lib = _lib.load()
        nbytes = workspace_bytes(lib, B, T, N, max_len)
        ws = workspace if workspace is not None and workspace.numel() >= nbytes else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.ishara_ctc_nbest_grad(_lib.ptr(x), B, T, Cn, blank, _lib.ptr(hyp_idx), _lib.ptr(hyp_len), N, Th, max_len, _lib.ptr(fl),
                                             _lib.ptr(coef), C_.c_float(grad_scale), _lib.ptr(out), 1 if accumulate else 0, _lib.ptr(dlb),
                                             _lib.ptr(logp), _lib.ptr(status), _lib.ptr(ws), _lib.stream()), "ishara_ctc_nbest_grad")
    return (out, logp, status) if return_logp else out


def launch_weights(lib, hyp_idx, hyp_len, logp, status, B: int, N: int, Th: int, targets, L: int, inv_temp, mode: int, dist, post, risk, coef,
                   tlen, stream) -> None:
    """One ishara_mwer_weights launch on `stream` (graph-capturable)."""
    from . import _lib
    _lib.check(lib.ishara_mwer_weights(_lib.ptr(hyp_idx), _lib.ptr(hyp_len), _lib.ptr(logp), _lib.ptr(status), B, N, Th, _lib.ptr(targets), L,
                                       _lib.ptr(inv_temp), mode, _lib.ptr(dist), _lib.ptr(post), _lib.ptr(risk), _lib.ptr(coef), _lib.ptr(tlen),
                                       stream), "ishara_mwer_weights")


def mwer_weights(hyp_idx, hyp_len, logp, targets, temperature=1.0, normalise: bool = True, status=None) -> dict:
    """Distances, posterior, risk and coef of every clip on the device (ishara_mwer_weights).  hyp_idx int32 [B, N, Th], hyp_len int32
    [B, N]; logp fp32 [B, N]: ctc_score_nbest's; targets int32 [B, L <= 64] padded with 59; temperature: a number > 0, or a one-element fp32
    device tensor holding 1 / temperature; normalise: divide the distance by the target's length; status: ctc_score_nbest's, or None.
    Runs on the current stream, nothing waits.  Returns dict(dist int32 [B, N], post fp32 [B, N], risk fp32 [B], coef fp32 [B, N],
    tlen int32 [B])."""
    import torch
    from . import _lib, mbr
    from .rescore import _cuda, _nbest
    hyp_idx, hyp_len, B, N, Th = _nbest(hyp_idx, hyp_len)
    dev = hyp_idx.device
    logp = _cuda(logp, torch.float32, (B, N), "logp")
    status = None if status is None else _cuda(status, torch.int32, (B, N), "status")
    targets = _cuda(targets, torch.int32, None, "targets")
    if targets.ndim != 2 or targets.shape[0] != B or not 1 <= targets.shape[1] <= MAX_TARGET_LEN:
        raise ValueError(f"targets must be [B={B}, L] with 1 <= L <= {MAX_TARGET_LEN}, got {tuple(targets.shape)}")
    if isinstance(temperature, torch.Tensor):
        it_d = _cuda(temperature, torch.float32, (1,), "temperature (a device tensor holds 1 / temperature)")
    else:
        it = mbr.inverse_temperature(temperature)
        it_d = None if it == 1.0 else torch.full((1,), it, dtype=torch.float32, device=dev)
    for t, what in ((logp, "logp"), (status, "status"), (targets, "targets"), (it_d, "temperature")):
        if t is not None and t.device != dev:
            raise ValueError(f"hyp_idx and {what} must be on one device")
    out = dict(dist=torch.empty((B, N), dtype=torch.int32, device=dev), post=torch.empty((B, N), dtype=torch.float32, device=dev),
               risk=torch.empty((B,), dtype=torch.float32, device=dev), coef=torch.empty((B, N), dtype=torch.float32, device=dev),
               tlen=torch.empty((B,), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        launch_weights(_lib.load(), hyp_idx, hyp_len, logp, status, B, N, Th, targets, int(targets.shape[1]), it_d, 1 if normalise else 0,
                       out["dist"], out["post"], out["risk"], out["coef"], out["tlen"], _lib.stream())
    return out


def mwer_max_len(target_width: int) -> int:
    """the longest hypothesis mwer_loss lets take part: twice the targets' width (at least 32), within the kernel's 255; a longer one is
    far from any target and leaves the list (status 8) rather than sizing the workspace"""
    return int(min(MAX_HYP_LEN, max(2 * int(target_width), 32)))


def nbest_pipeline(x, fl, targets59, beam_width: int, nbest: int, temperature, normalise: bool, blank: int, max_len: int, grad_scale: float,
                   want_grad: bool = True):
    """search -> exact scores -> weights -> one ctc_nbest_grad on the current stream: (risk [B], grad [B, T, C] or None, details)"""
    import torch
    from . import _lib, ctc_beam
    from .rescore import ctc_score_nbest
    B, T, Cn = x.shape
    ctc_beam.check_device_args(Cn, T, beam_width, nbest)
    lib = _lib.load()
    idx = torch.empty((B, nbest, T), dtype=torch.int32, device=x.device)
    ln = torch.empty((B, nbest), dtype=torch.int32, device=x.device)
    sc = torch.empty((B, nbest), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ws = torch.empty(max(ctc_beam.workspace_bytes(lib, B, T, Cn, beam_width), 4), dtype=torch.uint8, device=x.device)
        _lib.check(lib.ishara_ctc_beam_decode_ex(_lib.ptr(x), B, T, Cn, blank, beam_width, nbest, None, C_.c_float(0.0), C_.c_float(0.0), _lib.ptr(ws),
                                                 _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(fl), _lib.stream()), "ishara_ctc_beam_decode_ex")
    logp, status = ctc_score_nbest(x, idx, ln, fl, blank, return_status=True)
    status = torch.where(ln > max_len, torch.full_like(status, STATUS_LONG), status)      # what ishara_ctc_nbest_grad will say of the slot
    w = mwer_weights(idx, ln, logp, targets59, temperature, normalise, status)
    grad = ctc_nbest_grad(x, idx, ln, w["coef"], fl, grad_scale, max_len=max_len, blank=blank) if want_grad else None
    return w["risk"], grad, dict(w, hyp_idx=idx, hyp_len=ln, logp=logp, status=status)


class _MwerLossFn:
    """built on first use: torch is imported lazily in this module"""
    fn = None


def _mwer_fn():
    import torch
    if _MwerLossFn.fn is not None:
        return _MwerLossFn.fn

    class MwerLossFn(torch.autograd.Function):
        """forward: search, exact scores, weights and one ishara_ctc_nbest_grad with the reduction's factor in grad_scale; backward hands the
        saved gradient on.  The n-best list is a constant."""

        @staticmethod
        def forward(ctx, x, fl, targets59, beam_width, nbest, temperature, normalise, blank, max_len, reduction):
            B = x.shape[0]
            xc = x.detach()
            xc = xc if (xc.dtype == torch.float32 and xc.is_contiguous()) else xc.to(torch.float32).contiguous()
            need = ctx.needs_input_grad[0]
            scale = 1.0 / B if reduction == "mean" else 1.0
            risk, grad, _ = nbest_pipeline(xc, fl, targets59, beam_width, nbest, temperature, normalise, blank, max_len, scale, need)
            ctx.per_sample = reduction == "none"
            ctx.in_dtype = x.dtype
            if need:
                ctx.save_for_backward(grad)
            if reduction == "none":
                return risk
            return risk.sum() * scale

        @staticmethod
        def backward(ctx, g):
            (grad,) = ctx.saved_tensors
            if ctx.per_sample:
                grad = grad * g.to(grad.dtype)[:, None, None]
            elif float(g) != 1.0:                           # loss.backward() passes 1: the saved gradient is the answer as it is
                grad = grad * g.to(grad.dtype)
            return (grad.to(ctx.in_dtype),) + (None,) * 9

    _MwerLossFn.fn = MwerLossFn
    return MwerLossFn


def mwer_loss(log_probs, input_lengths, targets, target_lengths, beam_width: int = 8, nbest: int = 4, temperature: float = 1.0,
              normalise: bool = True, blank: int = 0, reduction: str = "mean"):
    """The expected edit distance over the model's own n-best list, for the torch families: differentiable with respect to log_probs
    [B, T, C] (fp32 on the GPU, logits or log-probabilities).  input_lengths [B] in 1..T; targets [B, S <= 64] integers with
    target_lengths [B] in 0..S (no target symbol may be 59 unless C > 59 makes it a class: the device's target rows are padded with 59, so
    a target holding 59 is cut there); beam_width / nbest: the search; temperature of the list's posterior; normalise: distances divided by
    the target's length; reduction "none" -> [B], "sum", or "mean" over the batch.  A clip without a live hypothesis gives NaN.  A
    hypothesis longer than mwer_max_len(S) leaves the list.  The n-best list is treated as a constant, as in the papers."""
    import torch
    from . import ctc, mbr
    x = ctc._logits(log_probs, "log_probs")
    B, T, Cn = x.shape
    if not 2 <= Cn <= MAX_CLASSES:
        raise ValueError(f"C={Cn} outside 2..{MAX_CLASSES} (one lane per class)")
    if not 0 <= int(blank) < Cn:
        raise ValueError(f"blank {blank} outside 0..{Cn - 1}")
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"reduction must be none / sum / mean, got {reduction!r}")
    tg = torch.as_tensor(targets)
    if tg.ndim != 2 or tg.shape[0] != B or not 1 <= tg.shape[1] <= MAX_TARGET_LEN:
        raise ValueError(f"targets must be [B={B}, S] with 1 <= S <= {MAX_TARGET_LEN}, got {tuple(tg.shape)}")
    S = tg.shape[1]
    fl = ctc._lengths(input_lengths, B, T, 1, "input_lengths", x.device)
    tl = ctc._lengths(target_lengths, B, S, 0, "target_lengths", x.device)
    mbr.inverse_temperature(temperature)                    # refuses a temperature that is not finite and > 0
    ctc._need_gpu(x, "log_probs")
    t59 = ctc.pack_targets(tg, tl, 59, x.device).to(torch.int32).contiguous()
    return _mwer_fn().apply(x, fl, t59, int(beam_width), int(nbest), float(temperature), bool(normalise), int(blank), mwer_max_len(S), reduction)
