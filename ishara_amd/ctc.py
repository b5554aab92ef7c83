"""CTC on batches whose clips have different frame counts: the loss, the greedy decoder, the prefix beam search and the forced aligner over
the `*_ex` entry points of include/ishara_hip.h (csrc/ctc.hip, ctc_beam.hip, ctc_align.hip).

The torch families return `(log_probs [B, T, C], output_lengths)`; every function here takes that pair as it comes: batch-first, no
transposed copy, and a length tensor that already lives on the device is handed to the kernel without a host round trip.  The rule of the
kernels: the buffer's T is a stride, sample b uses its first `lengths[b]` frames only and computes bit for bit what the
fixed-T entry point computes on `x[b:b+1, :lengths[b]]`; rows past a sample's end are never read.

Lengths given as a list, a numpy array or a CPU tensor are validated here (1 .. T).  A device tensor is not looked at (that would
synchronise): the kernel treats a value outside 1 .. T as a sample without frames (loss: inf, or 0 with zero_infinity; decoders: nothing
decoded; aligner: no alignment).

Kernel limits: C <= 64 classes, target rows of at most 255 symbols, T <= 4096 for the decoders and the aligner.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Tuple

import numpy as np
import torch

from . import _lib

MAX_CLASSES = 64
MAX_TARGET = 255
ZERO_INFEASIBLE = 1        # ISHARA_CTC_ZERO_INFEASIBLE
SENTINEL = 1e29            # nll >= SENTINEL: the sample has no alignment (the kernel writes 1e30)


def _lengths(v, B: int, hi: int, lo: int, what: str, device) -> torch.Tensor:
    """`v` as a contiguous int32 [B] tensor on `device`; validated against lo .. hi when it lives on the host."""
    t = v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))
    if t.dtype.is_floating_point or t.dtype == torch.bool or t.ndim != 1 or t.shape[0] != B:
        raise ValueError(f"{what} must be {B} integers, got {tuple(t.shape)} {t.dtype}")
    if t.device.type == "cpu" and B > 0:
        mn, mx = int(t.min()), int(t.max())
        if mn < lo or mx > hi:
            raise ValueError(f"{what} must lie in {lo}..{hi}, got {mn}..{mx}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _logits(x, what: str = "logits") -> torch.Tensor:
    x = torch.as_tensor(x)
    if x.ndim != 3:
        raise ValueError(f"{what} must be [B, T, C], got {tuple(x.shape)}")
    return x


def _need_gpu(x, what: str = "logits") -> None:
    if not x.is_cuda:
        raise _lib.IsharaError(f"{what} must be on the GPU: the CTC kernels have no CPU path")


def pack_targets(targets, target_lengths, blank: int, device) -> torch.Tensor:
    """targets [B, S] + target_lengths [B] -> the kernel's label rows [B, max(S, 1)] int64, `blank` from each row's length on."""
    t = torch.as_tensor(targets).to(device=device, dtype=torch.int64)
    B, S = t.shape
    if S == 0:
        return torch.full((B, 1), blank, dtype=torch.int64, device=device)
    keep = torch.arange(S, device=device)[None, :] < target_lengths.to(device)[:, None]
    return torch.where(keep, t, torch.full_like(t, blank)).contiguous()


class _CtcLossFn(torch.autograd.Function):
    """forward: one ishara_ctc_loss_ex launch computes nll [B] and, when a gradient is wanted, dlogits with the reduction's per-sample weight
    already in it (sample_scale); backward hands the saved gradient on."""

    @staticmethod
    def forward(ctx, x, labels, frame_len, weight, blank, zero_infinity, reduction):
        lib = _lib.load()
        B, T, Cc = x.shape
        L = labels.shape[1]
        xc = x.detach()
        xc = xc if (xc.dtype == torch.float32 and xc.is_contiguous()) else xc.to(torch.float32).contiguous()
        need = ctx.needs_input_grad[0]
        nll = torch.empty(B, dtype=torch.float32, device=x.device)
        grad = torch.empty((B, T, Cc), dtype=torch.float32, device=x.device) if need else None
        if B > 0:
            with torch.cuda.device(x.device):
                ws = torch.empty(int(lib.ishara_ctc_workspace_bytes(B, T, L)), dtype=torch.uint8, device=x.device)
                _lib.check(lib.ishara_ctc_loss_ex(_lib.ptr(xc), _lib.ptr(labels), B, T, Cc, L, blank, _lib.ptr(nll), _lib.ptr(grad), C.c_float(1.0),
                                                  _lib.ptr(ws), _lib.ptr(frame_len), _lib.ptr(weight), ZERO_INFEASIBLE if zero_infinity else 0,
                                                  _lib.stream()), "ishara_ctc_loss_ex")
        ctx.per_sample = reduction == "none"
        ctx.in_dtype = x.dtype
        if need:
            ctx.save_for_backward(grad)
        nll = torch.where(nll >= SENTINEL, torch.full_like(nll, 0.0 if zero_infinity else float("inf")), nll)
        if reduction == "none":
            return nll
        return (nll * weight).sum() if weight is not None else nll.sum()

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        if ctx.per_sample:
            grad = grad * g.to(grad.dtype)[:, None, None]
        elif float(g) != 1.0:                               # loss.backward() passes 1: the saved gradient is the answer as it is
            grad = grad * g.to(grad.dtype)
        return grad.to(ctx.in_dtype), None, None, None, None, None, None


def ctc_loss(log_probs, targets, input_lengths, target_lengths, blank: int = 0, reduction: str = "mean", zero_infinity: bool = False
             ) -> torch.Tensor:
    """`torch.nn.functional.ctc_loss` for batch-first input, on the library's own kernel.

    log_probs [B, T, C] fp32 on the GPU: logits or log-probabilities (the kernel takes the log-softmax of each row, which leaves a
    normalised row as it is).  targets [B, S] integers, target_lengths [B] in 0..S, input_lengths [B] in 1..T.  reduction "none" -> [B],
    "sum", or "mean" = mean over the batch of nll_b / max(target_lengths[b], 1), as torch defines it.  A sample whose target does not
    fit its own length gives inf, or 0 with a zero gradient under zero_infinity.  Differentiable with respect to log_probs; the gradient
    past a sample's length is exactly 0.  Limits: C <= 64, S <= 255 (ValueError)."""
    x = _logits(log_probs, "log_probs")
    B, T, Cc = x.shape
    if not 2 <= Cc <= MAX_CLASSES:
        raise ValueError(f"C={Cc} outside 2..{MAX_CLASSES} (one lane per class)")
    if not 0 <= int(blank) < Cc:
        raise ValueError(f"blank {blank} outside 0..{Cc - 1}")
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"reduction must be none / sum / mean, got {reduction!r}")
    tg = torch.as_tensor(targets)
    if tg.ndim != 2 or tg.shape[0] != B:
        raise ValueError(f"targets must be [B={B}, S], got {tuple(tg.shape)}")
    S = tg.shape[1]
    if S > MAX_TARGET:
        raise ValueError(f"S={S} target symbols per row, the kernel takes at most {MAX_TARGET}")
    fl = _lengths(input_lengths, B, T, 1, "input_lengths", x.device)
    tl = _lengths(target_lengths, B, S, 0, "target_lengths", x.device)
    _need_gpu(x, "log_probs")                               # after the host validation: a bad argument is reported as such everywhere
    labels = pack_targets(tg, tl, int(blank), x.device)
    weight = (1.0 / (B * tl.clamp(min=1).to(torch.float32))).contiguous() if reduction == "mean" and B > 0 else None
    return _CtcLossFn.apply(x, labels, fl, weight, int(blank), bool(zero_infinity), reduction)


def _ragged(x, lengths) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    x = _logits(x)
    fl = None if lengths is None else _lengths(lengths, x.shape[0], x.shape[1], 1, "lengths", x.device)
    _need_gpu(x)
    return x.to(torch.float32).contiguous(), fl


def ctc_greedy_decode(logits, lengths=None, blank: Optional[int] = None) -> List[np.ndarray]:
    """decode_phrase of every clip's first `lengths[b]` frames (the run ending at the clip's last frame is never emitted, as in the
    reference) -> list of int64 index arrays, what `Model.decode_batch` returns.  blank defaults to C - 1."""
    idx, ln = greedy_decode_device(logits, lengths, blank)
    idx, ln = idx.cpu().numpy(), ln.cpu().numpy()
    return [idx[b, :ln[b]].astype(np.int64) for b in range(idx.shape[0])]


def greedy_decode_device(logits, lengths=None, blank: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The same decode left on the device: (indices int32 [B, T], lengths int32 [B]), the layout ishara_edit_distance / ishara_edit_alignment read."""
    x, fl = _ragged(logits, lengths)
    B, T, Cc = x.shape
    blank = Cc - 1 if blank is None else int(blank)
    idx = torch.empty((B, T), dtype=torch.int32, device=x.device)
    ln = torch.empty(B, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ishara_greedy_decode_ex(_lib.ptr(x), B, T, Cc, blank, _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(fl), _lib.stream()),
                   "ishara_greedy_decode_ex")
    return idx, ln


def ctc_beam_decode(logits, lengths=None, beam_width: int = 16, nbest: int = 1, lm=None, alpha: float = 0.0, beta: float = 0.0,
                    workspace: Optional[torch.Tensor] = None) -> List[List[Tuple[np.ndarray, float]]]:
    """CTC prefix beam search (ishara_amd/ctc_beam.py semantics, blank = C - 1) of every clip's first `lengths[b]` frames -> per clip a
    list of (indices int64, score), best first: what `Model.beam_decode` returns.  lm: None, a [C, C] table / CharBigramLM, or a
    CharNGramLM / LMAutomaton (ctc_lm.py, launched as ishara_ctc_beam_decode_lm).  `workspace`: a uint8 device tensor to reuse, if large enough."""
    from . import ctc_beam
    x, fl = _ragged(logits, lengths)
    B, T, Cc = x.shape
    ctc_beam.check_device_args(Cc, T, beam_width, nbest)
    lm_dev = ctc_beam.lm_to_device(lm, Cc, x.device)
    lib = _lib.load()
    nbytes = max(ctc_beam.workspace_bytes(lib, B, T, Cc, beam_width), 4)
    ws = workspace if workspace is not None and workspace.numel() >= nbytes else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    idx = torch.empty((B, nbest, T), dtype=torch.int32, device=x.device)
    ln = torch.empty((B, nbest), dtype=torch.int32, device=x.device)
    sc = torch.empty((B, nbest), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ctc_beam.launch(lib, x, B, T, Cc, beam_width, nbest, lm_dev, alpha, beta, ws, idx, ln, sc, _lib.stream(), frame_len=fl, ex=True)
    idx, ln, sc = idx.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()
    return [[(idx[b, n, :ln[b, n]].astype(np.int64), float(sc[b, n])) for n in range(nbest) if ln[b, n] >= 0] for b in range(B)]


def ctc_beam_nbest_device(logits, lengths=None, beam_width: int = 16, nbest: int = 8, lm=None, alpha: float = 0.0, beta: float = 0.0,
                          workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The same search left on the device: (indices int32 [B, nbest, T] padded with -1, lengths int32 [B, nbest] with -1 in a slot without
    a hypothesis, scores fp32 [B, nbest] with -inf there), ranked best first: what `mbr.mbr_select` and `mbr.pool_nbest` read.  Launched on
    the current stream; nothing waits."""
    from . import ctc_beam
    x, fl = _ragged(logits, lengths)
    B, T, Cc = x.shape
    ctc_beam.check_device_args(Cc, T, beam_width, nbest)
    lm_dev = ctc_beam.lm_to_device(lm, Cc, x.device)
    lib = _lib.load()
    nbytes = max(ctc_beam.workspace_bytes(lib, B, T, Cc, beam_width), 4)
    ws = workspace if workspace is not None and workspace.numel() >= nbytes else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    idx = torch.empty((B, nbest, T), dtype=torch.int32, device=x.device)
    ln = torch.empty((B, nbest), dtype=torch.int32, device=x.device)
    sc = torch.empty((B, nbest), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        ctc_beam.launch(lib, x, B, T, Cc, beam_width, nbest, lm_dev, alpha, beta, ws, idx, ln, sc, _lib.stream(), frame_len=fl, ex=True)
    del ws        # the caching allocator hands the block out again in stream order: the kernel has read it by then
    return idx, ln, sc


def ctc_align(logits, labels, lengths=None, blank: Optional[int] = None, workspace: Optional[torch.Tensor] = None) -> list:
    """CTC forced alignment (ishara_amd/ctc_align.py semantics) of every clip's first `lengths[b]` frames to labels [B, L] padded with
    blank (default C - 1) -> per clip an Alignment, what `Model.align` returns; frame_pos keeps the buffer's T entries, -1 past the clip."""
    from . import ctc_align as A
    x, fl = _ragged(logits, lengths)
    y = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor) else labels).to(x.device, torch.int64).contiguous()
    if y.ndim != 2 or y.shape[0] != x.shape[0]:
        raise ValueError(f"logits must be [B, T, C] and labels [B, L], got {tuple(x.shape)} and {tuple(y.shape)}")
    B, T, Cc = x.shape
    L = y.shape[1]
    blank = Cc - 1 if blank is None else int(blank)
    A.check_device_args(Cc, T, L, blank)
    lib = _lib.load()
    nbytes = max(A.workspace_bytes(lib, B, T, L), 16)
    ws = workspace if workspace is not None and workspace.numel() >= nbytes else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    fp = torch.empty((B, T), dtype=torch.int32, device=x.device)
    st = torch.empty((B, L), dtype=torch.int32, device=x.device)
    en = torch.empty((B, L), dtype=torch.int32, device=x.device)
    cf = torch.empty((B, L), dtype=torch.float32, device=x.device)
    sc = torch.empty(B, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        A.launch(lib, x, y, B, T, Cc, L, blank, ws, fp, st, en, cf, sc, _lib.stream(), frame_len=fl, ex=True)
    return A.to_alignments(y.cpu().numpy(), *(t.cpu().numpy() for t in (fp, st, en, cf, sc)))


# ---------------------------------------------------------------------------------------------------- host references of a ragged batch
def ragged_clips(logits, lengths) -> List[np.ndarray]:
    """The clips a ragged batch stands for: logits[b, :lengths[b]].  The host references (`prefix_beam_search`, `viterbi_align`) take one
    clip; the reference of a ragged batch is the loop over these."""
    x = np.asarray(logits)
    return [x[b, :int(n)] for b, n in enumerate(np.asarray(lengths))]


def prefix_beam_search_ragged(logits, lengths, beam_width: int, **kw) -> list:
    from .ctc_beam import prefix_beam_search
    return [prefix_beam_search(c, beam_width, **kw) for c in ragged_clips(logits, lengths)]


def viterbi_align_ragged(logits, labels, lengths, blank: int):
    """`viterbi_align` clip by clip, returned in the batched layout with frame_pos padded with -1 to the buffer's T."""
    from .ctc_align import viterbi_align
    x, y = np.asarray(logits, np.float32), np.asarray(labels, np.int64)
    B, T, L = x.shape[0], x.shape[1], y.shape[1]
    fp = np.full((B, T), -1, np.int32)
    st, en = np.full((B, L), -1, np.int32), np.full((B, L), -1, np.int32)
    cf, sc = np.zeros((B, L), np.float64), np.zeros(B, np.float64)
    for b, c in enumerate(ragged_clips(x, lengths)):
        f, st[b], en[b], cf[b], sc[b] = viterbi_align(c, y[b], blank)
        fp[b, :len(f)] = f
    return fp, st, en, cf, sc
