"""Knowledge distillation of a teacher's frame posteriors into the training step: the host definition and the device entries of
`ishara_kd_grad` (csrc/kd_grad.hip) and `ishara_loss_backward_kd` (csrc/keras_hybrid.hip); contracts in include/ishara_hip.h.

The serving side fuses several models (ensemble.py, rescore.py); the deployed artefact stays one small model.  Distillation (Hinton et al.
2015) trains that model on the teacher's softened class posteriors beside the label, frame by frame:

  student   ps = softmax(z / tau), the step's own logits z [B, T, C]
  teacher   pt = softmax(u / tau), u the teacher's rows: raw logits or normalised log-probabilities (combine_logits' output); a constant
  loss      tau^2 * KL(pt || ps) per frame, summed (or, with normalise, averaged) over the clip's frames, averaged over the batch, times
            kd_weight, beside kd_ctc_weight * CTC
  gradient  d (tau^2 KL) / d z = tau * (ps - pt): one ishara_kd_grad call, added into the CTC gradient between the loss kernel and the head

  kd_reference                                  the definition in numpy fp64
  kd_grad                                       device tensors in, device tensors out, on the current stream, nothing waits
  kd_loss                                       a torch.autograd.Function for the torch families
  Optimizer(kd_weight=...) / Model.set_teacher  the Keras-hybrid family's training step (model.py); Model.kd_stats reads the last KL

The teacher must share the student's T and alphabet; sequence-level distillation from an n-best list and hidden-state distillation are not
built.  In the Keras family the term keeps logit_length = T as the CTC loss does.  No accuracy effect is measured anywhere in this
repository: there is no dataset and there are no trained weights.
"""
from __future__ import annotations

import ctypes as C_
import math
from typing import Optional

import numpy as np

MAX_CLASSES, MAX_FRAMES, MAX_BATCH = 64, 4096, 65535
MODES = {"sum": 0, "mean": 1}
OPTION_NAMES = ("kd_weight", "kd_temperature", "kd_ctc_weight", "kd_normalise", "kd_start_step")


def _mode(mode) -> int:
    if mode in (0, 1) and not isinstance(mode, bool):
        return int(mode)
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)} (or 0 / 1), got {mode!r}")
    return MODES[mode]


def inverse_temperature(temperature, what: str = "temperature") -> float:
    """1 / tau as the float32 value the device multiplies by; a temperature that is not a finite number > 0 is refused"""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.integer, np.floating)) or not math.isfinite(float(temperature)) \
            or float(temperature) <= 0:
        raise ValueError(f"{what} must be a finite number > 0, got {temperature!r}")
    with np.errstate(over="ignore", under="ignore"):
        it = float(np.float32(1.0 / float(temperature)))
    if not (math.isfinite(it) and it > 0):
        raise ValueError(f"{what} {temperature!r} has no float32 inverse > 0")
    return it


def clip_frames(frame_lengths, B: int, T: int) -> np.ndarray:
    """Tb per clip: T without lengths, 0 for a value outside [1, T]"""
    if frame_lengths is None:
        return np.full(B, T, np.int64)
    fl = np.asarray(frame_lengths).astype(np.int64)
    if fl.shape != (B,):
        raise ValueError(f"frame_lengths must be {B} integers, got shape {fl.shape}")
    return np.where((fl < 1) | (fl > T), 0, fl)


# ---------------------------------------------------------------------------------------------------- host reference
def _softmax64(z):
    d = z - z.max(axis=-1, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=-1, keepdims=True)
    return d - np.log(s), e / s


def kd_reference(logits, teacher, inv_temp: float = 1.0, mode="sum", frame_lengths=None, grad_scale: float = 1.0) -> dict:
    """The definition in numpy fp64.  logits, teacher [B, T, C]; inv_temp and grad_scale are taken at their float32 values, as the device
    gets them; mode "sum" (0) or "mean" (1): w_b = 1 or 1 / Tb; frame_lengths: B integers, a value outside [1, T] means a clip without
    frames; rows past a clip's end are read from neither input (they may hold NaN) and give 0.
    Returns dict(grad [B, T, C] = grad_scale * w_b * (ps - pt), kl_frame [B, T] = sum_c pt * (log pt - log ps), kl_clip [B] = the sum of
    kl_frame (mode 1: times 1 / Tb), frames [B] = Tb, w [B] = w_b)."""
    md = _mode(mode)
    z = np.asarray(logits)
    u = np.asarray(teacher)
    if z.ndim != 3 or u.shape != z.shape:
        raise ValueError(f"logits and teacher must be [B, T, C] of one shape, got {z.shape} and {u.shape}")
    B, T, Cn = z.shape
    it, gs = float(np.float32(inv_temp)), float(np.float32(grad_scale))
    tb = clip_frames(frame_lengths, B, T)
    inside = np.arange(T)[None, :] < tb[:, None]
    z64 = np.where(inside[..., None], z.astype(np.float64), 0.0) * it
    u64 = np.where(inside[..., None], u.astype(np.float64), 0.0) * it
    lps, ps = _softmax64(z64)
    lpt, pt = _softmax64(u64)
    w = np.where(tb > 0, 1.0 / np.maximum(tb, 1), 0.0) if md == 1 else np.ones(B)
    grad = np.where(inside[..., None], gs * (w[:, None, None] * (ps - pt)), 0.0)
    kl_frame = np.where(inside, (pt * (lpt - lps)).sum(axis=-1), 0.0)
    kl_clip = kl_frame.sum(axis=1) * (w if md == 1 else 1.0)
    return dict(grad=grad, kl_frame=kl_frame, kl_clip=kl_clip, frames=tb, w=w)


# ---------------------------------------------------------------------------------------------------- options of the training step
def check_options(kd_weight=0.0, kd_temperature=2.0, kd_ctc_weight=1.0, kd_normalise=True, kd_start_step=0) -> dict:
    """The five Optimizer(kd_*) options, validated; returns them as a plain dict (the optional key of save_state)."""

    def number(v, what, positive=False):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) or float(v) < 0 or (
                positive and float(v) == 0):
            raise ValueError(f"{what} must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
        return float(v)

    tau = number(kd_temperature, "kd_temperature", positive=True)
    inverse_temperature(tau, "kd_temperature")
    if not isinstance(kd_normalise, (bool, np.bool_)):
        raise ValueError(f"kd_normalise must be True or False, got {kd_normalise!r}")
    if isinstance(kd_start_step, bool) or not isinstance(kd_start_step, (int, np.integer)) or not 0 <= int(kd_start_step) <= 2 ** 31 - 1:
        raise ValueError(f"kd_start_step must be an integer in 0..{2 ** 31 - 1}, got {kd_start_step!r}")
    return dict(kd_weight=number(kd_weight, "kd_weight"), kd_temperature=tau, kd_ctc_weight=number(kd_ctc_weight, "kd_ctc_weight"),
                kd_normalise=bool(kd_normalise), kd_start_step=int(kd_start_step))


# ---------------------------------------------------------------------------------------------------- device side
def _rows(t, what: str):
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a torch tensor on the GPU, got {type(t).__name__}")
    if not t.is_cuda:
        from . import _lib
        raise _lib.IsharaError(f"{what} must be on the GPU: the distillation kernel has no CPU path (kd_reference is the host definition)")
    if t.ndim != 3:
        raise ValueError(f"{what} must be [B, T, C], got {tuple(t.shape)}")
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def _frame_len(lengths, B: int, device):
    """int32 [B] on the device; the values are not checked: a value outside [1, T] means a clip without frames"""
    import torch
    if lengths is None:
        return None
    t = lengths if isinstance(lengths, torch.Tensor) else torch.as_tensor(np.asarray(lengths))
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.ndim != 1 or t.shape[0] != B:
        raise ValueError(f"lengths must be {B} integers, got {tuple(t.shape)} {t.dtype}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def kd_grad(logits, teacher, lengths=None, inv_temp: float = 1.0, mode="sum", grad_scale: float = 1.0, out=None, accumulate: bool = False,
            dlb=None, return_kl: bool = False):
    """grad_scale * w_b * (softmax(logits * inv_temp) - softmax(teacher * inv_temp)) on the device (ishara_kd_grad).  logits, teacher fp32
    [B, T, C] on one GPU (teacher may be logits itself); lengths: the clips' frame counts (None: T each; a value outside [1, T]: no frames);
    mode "sum" / "mean" over the clip's frames; out: the fp32 [B, T, C] tensor to write (None: a new one; with accumulate the sum out + G is
    written, rows past a clip's end stay); dlb: an int32 [B * T, 64] tensor for the padded bf16 copy of the final rows, or None.  Runs on the
    current stream, nothing waits.  Returns the gradient tensor; with return_kl (G, kl_frame fp32 [B, T], kl_clip fp32 [B])."""
    import torch
    from . import _lib
    md = _mode(mode)
    x = _rows(logits, "logits")
    u = x if teacher is logits else _rows(teacher, "teacher")
    if u.shape != x.shape:
        raise ValueError(f"teacher must have the logits' shape {tuple(x.shape)}, got {tuple(u.shape)}")
    B, T, Cn = x.shape
    if not 2 <= Cn <= MAX_CLASSES:
        raise ValueError(f"C={Cn} outside 2..{MAX_CLASSES} (one lane per class)")
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"T={T} outside 1..{MAX_FRAMES}")
    if B > MAX_BATCH:
        raise ValueError(f"B={B} > {MAX_BATCH}")
    if accumulate and out is None:
        raise ValueError("accumulate adds into out=: give the tensor")
    if out is None:
        out = torch.empty((B, T, Cn), dtype=torch.float32, device=x.device)
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (B, T, Cn) and out.is_contiguous()):
        raise ValueError(f"out must be a contiguous fp32 [{B}, {T}, {Cn}] tensor on the GPU")
    if dlb is not None and not (isinstance(dlb, torch.Tensor) and dlb.is_cuda and dlb.dtype == torch.int32 and tuple(dlb.shape) == (B * T, 64)
                                and dlb.is_contiguous()):
        raise ValueError(f"dlb must be a contiguous int32 [{B * T}, 64] tensor on the GPU")
    for t, what in ((u, "teacher"), (out, "out"), (dlb, "dlb")):
        if t is not None and t.device != x.device:
            raise ValueError(f"logits and {what} must be on one device")
    fl = _frame_len(lengths, B, x.device)
    klf = torch.empty((B, T), dtype=torch.float32, device=x.device) if return_kl else None
    klc = torch.empty((B,), dtype=torch.float32, device=x.device) if return_kl else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ishara_kd_grad(None, _lib.ptr(x), _lib.ptr(u), B, T, Cn, C_.c_float(inv_temp), md, _lib.ptr(fl), C_.c_float(grad_scale),
                                              _lib.ptr(out), 1 if accumulate else 0, _lib.ptr(dlb), _lib.ptr(klf), _lib.ptr(klc), _lib.stream()),
                   "ishara_kd_grad")
    return (out, klf, klc) if return_kl else out


class _KdLossFn:
    """built on first use: torch is imported lazily in this module"""
    fn = None


def _kd_fn():
    import torch
    if _KdLossFn.fn is not None:
        return _KdLossFn.fn

    class KdLossFn(torch.autograd.Function):
        """forward: one ishara_kd_grad launch for kl_clip; backward: one launch with tau and the reduction's factor in grad_scale, times the
        incoming gradient on the device.  The teacher is a constant."""

        @staticmethod
        def forward(ctx, x, u, fl, inv_temp, tau, mode, reduction):
            B = x.shape[0]
            xc = _rows(x.detach(), "logits")
            _, _, klc = kd_grad(xc, u, fl, inv_temp, mode, 0.0, return_kl=True)
            ctx.save_for_backward(xc, u)
            ctx.fl, ctx.inv_temp, ctx.tau, ctx.mode, ctx.in_dtype = fl, inv_temp, tau, mode, x.dtype
            ctx.per_sample = reduction == "none"
            ctx.factor = 1.0 / B if reduction == "mean" else 1.0
            per_clip = klc * (tau * tau)
            return per_clip if reduction == "none" else per_clip.sum() * ctx.factor

        @staticmethod
        def backward(ctx, g):
            xc, u = ctx.saved_tensors
            grad = kd_grad(xc, u, ctx.fl, ctx.inv_temp, ctx.mode, ctx.tau * ctx.factor)
            g = g.to(grad.dtype)
            grad = grad * (g[:, None, None] if ctx.per_sample else g)
            return (grad.to(ctx.in_dtype),) + (None,) * 6

    _KdLossFn.fn = KdLossFn
    return KdLossFn


def kd_loss(logits, teacher, output_lengths=None, temperature: float = 1.0, normalise: bool = True, reduction: str = "mean"):
    """tau^2 * KL(softmax(teacher / tau) || softmax(logits / tau)) per clip, for the torch families: differentiable with respect to logits
    [B, T, C] (fp32 on the GPU, logits or log-probabilities); teacher [B, T, C] is a constant (logits or log-probabilities).
    output_lengths [B]: the clips' frame counts (None: T each); normalise: the clip's mean over its frames, else its sum; reduction "none"
    -> [B], "sum", or "mean" over the batch."""
    import torch
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"reduction must be none / sum / mean, got {reduction!r}")
    if not isinstance(normalise, (bool, np.bool_)):
        raise ValueError(f"normalise must be True or False, got {normalise!r}")
    it = inverse_temperature(temperature)
    x = torch.as_tensor(logits)
    if x.ndim != 3:
        raise ValueError(f"logits must be [B, T, C], got {tuple(x.shape)}")
    u = _rows(torch.as_tensor(teacher).detach(), "teacher")
    if u.shape != x.shape:
        raise ValueError(f"teacher must have the logits' shape {tuple(x.shape)}, got {tuple(u.shape)}")
    if not x.is_cuda:
        _rows(x, "logits")
    fl = _frame_len(output_lengths, x.shape[0], x.device)
    return _kd_fn().apply(x, u, fl, it, float(temperature), 1 if normalise else 0, reduction)
