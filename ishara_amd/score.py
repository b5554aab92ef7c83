"""Edit-operation alignment of device decodes (csrc/score_align.hip, ishara_edit_alignment): which characters a decode confuses, drops
or hallucinates, for the output of any decoder that writes the greedy layout (indices int32 [B, T], lengths int32 [B]).

The definitions are those of `evaluation.edit_alignment` (the host yardstick): every output is an integer and equals it exactly.
`BatchedTFLiteModel.score(breakdown=True)` captures the same kernel into its graph; `CallbackEval(error_report=True)` calls this entry.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib

MAX_LABEL_LEN = 64         # one wavefront lane per target symbol
MAX_FRAMES = 4096
N_SYM = 60                 # confusion matrix side: 59 characters and "nothing"


def _int32_cuda(t, ndim: int, what: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a torch tensor on the GPU, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what} must be on the GPU (the alignment kernel has no CPU path; evaluation.edit_alignment is the host reference)")
    if t.dtype != torch.int32:
        raise ValueError(f"{what} must be int32, got {t.dtype}")
    if t.ndim != ndim:
        raise ValueError(f"{what} must have {ndim} dimension{'s' if ndim > 1 else ''}, got {tuple(t.shape)}")
    return t.contiguous()


def workspace_bytes(B: int, T: int) -> int:
    return int(_lib.load().ishara_edit_alignment_workspace_bytes(B, T))


def edit_alignment_device(idx, lengths, targets, fallback: bool = False, confusion: Optional[torch.Tensor] = None,
                          workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """idx int32 [B, T] and lengths int32 [B] (ishara_greedy_decode's outputs, or the beam's top-1), targets int32 [B, L] padded with 59
    -> (ops [B, 4] = matches, substitutions, deletions, insertions; aligned [B, L]; inserted [B, L + 1]; confusion [60, 60]), device int32.
    confusion: a matrix to add to (sum a test set on the device), or None for a fresh zeroed one.  fallback: apply the TFLite wrapper's
    len < 3 rule first.  workspace: a uint8 device tensor of at least workspace_bytes(B, T) bytes to reuse, else one is allocated.  The
    launch is on the current stream; nothing waits."""
    idx = _int32_cuda(idx, 2, "idx")
    lengths = _int32_cuda(lengths, 1, "lengths")
    targets = _int32_cuda(targets, 2, "targets")
    B, T = idx.shape
    L = targets.shape[1]
    if lengths.shape[0] != B or targets.shape[0] != B:
        raise ValueError(f"idx [B={B}, T], lengths [B] and targets [B, L] disagree: {tuple(lengths.shape)}, {tuple(targets.shape)}")
    if L < 1 or L > MAX_LABEL_LEN:
        raise ValueError(f"L={L} target symbols per row outside 1..{MAX_LABEL_LEN} (one wavefront lane per target symbol)")
    if T < 1 or T > MAX_FRAMES:
        raise ValueError(f"T={T} outside 1..{MAX_FRAMES}")
    dev = idx.device
    if lengths.device != dev or targets.device != dev:
        raise ValueError("idx, lengths and targets must be on one device")
    if confusion is None:
        confusion = torch.zeros((N_SYM, N_SYM), dtype=torch.int32, device=dev)
    else:
        confusion = _int32_cuda(confusion, 2, "confusion")
        if tuple(confusion.shape) != (N_SYM, N_SYM) or confusion.device != dev or not confusion.is_contiguous():
            raise ValueError(f"confusion must be a contiguous [{N_SYM}, {N_SYM}] int32 tensor on {dev}")
    lib = _lib.load()
    need = int(lib.ishara_edit_alignment_workspace_bytes(B, T))
    if workspace is None:
        keep, ws = _lib.aligned(need, dev)
    else:
        if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.device != dev or workspace.dtype != torch.uint8:
            raise ValueError(f"workspace must be a uint8 tensor on {dev}")
        pad = (-workspace.data_ptr()) % 16
        if workspace.numel() - pad < need:
            raise ValueError(f"workspace of {workspace.numel()} bytes is too small: {need} bytes needed (16-byte aligned)")
        keep, ws = workspace, C.c_void_p(workspace.data_ptr() + pad)
    ops = torch.empty((B, 4), dtype=torch.int32, device=dev)
    aligned = torch.empty((B, L), dtype=torch.int32, device=dev)
    inserted = torch.empty((B, L + 1), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.ishara_edit_alignment(_lib.ptr(idx), _lib.ptr(lengths), B, T, _lib.ptr(targets), L, 1 if fallback else 0, _lib.ptr(ops),
                                             _lib.ptr(aligned), _lib.ptr(inserted), _lib.ptr(confusion), ws, _lib.stream()), "ishara_edit_alignment")
    del keep      # the caching allocator hands the block out again in stream order: the kernel has read it by then
    return ops, aligned, inserted, confusion
