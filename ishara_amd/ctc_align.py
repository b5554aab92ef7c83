"""CTC forced alignment: which frames spell which symbol of a known label.  The host reference of `ishara_ctc_align` (csrc/ctc_align.hip).

The loss, the greedy decoder and the beam search answer "what was spelled"; the alignment answers "when": the best single path through
the CTC lattice of a given label (Viterbi), cut into one frame span per symbol, each with a confidence.  The semantics below are
implemented exactly by both this module (numpy, fp64) and the kernel; every integer output of the two is equal on every input.

Inputs: logits [B, T, C] fp32, finite; labels [B, L] int64 padded with `blank`.  len_b is the number of entries before the first `blank`
of row b; what follows it is ignored.

Lattice: S = 2 len + 1 states, ext[s] = blank for even s and labels[s >> 1] for odd s.  Transitions are the CTC ones: stay, s-1 -> s, and
s-2 -> s only when ext[s] != blank and ext[s] != ext[s-2].

Best path: the one that maximises V = sum_t logits[t, ext[s_t]] -- on the RAW logits, not on their log-softmax: the log-sum-exp of a
frame is the same for every path and cannot change the argmax.  V is carried in IEEE fp64, v_t[s] = max(pred) + (double)logits[t, ext[s]],
one fp64 add per frame, in frame order.  Device and host do the same operations in the same order, so they hold bit-identical v and the
path is exact: no near-tie allowance.

Tie order: a predecessor replaces the current choice only if it is strictly greater, tried in the order stay, s-1, s-2 (on equality stay
wins, then s-1).  At the last frame the path ends in S-1, unless v[S-2] is strictly greater and len > 0.

Start: v_0[0] = logits[0, blank]; v_0[1] = logits[0, ext[1]] if len > 0; every other state is dead (-inf: it never wins a comparison
against a live state and never becomes live by an addition).

Infeasible samples: T < len + repeats (repeats = the i in [1, len) with labels[i] == labels[i-1]), or a label before the first blank
outside [0, C) -- the rule of `ishara_ctc_loss`.  An out-of-range label is read as blank and never used as an index.

Outputs per sample:
  frame_pos [T] int32   the label index i emitted at frame t, -1 on a blank frame
  start, end [L] int32  symbol i occupies frames [start, end), end > start; both -1 for i >= len
  conf [L] fp32         the mean over the span of softmax(logits[t])[labels[i]], each term expf(x - m) / sum_c expf(x_c - m) with m the row
                        maximum; 0 for i >= len
  score fp32            the log-probability of the best path, (V - sum_t m_t) - sum_t logf(sum_c expf(x_c - m_t)), both sums in fp64 (a
                        constant shift of the logits costs no precision)
An infeasible sample gets score = -1e30, frame_pos = -1, start = end = -1, conf = 0; the other samples' outputs are bit-identical to a
launch without it.
"""
from __future__ import annotations

from typing import List, NamedTuple, Tuple

import numpy as np

MAX_CLASSES = 64          # kernel limits (include/ishara_hip.h)
MAX_LABEL = 255
MAX_FRAMES = 4096
INFEASIBLE_SCORE = -1e30
BP_ROW_BYTES = 128        # back-pointers of one frame: 64 lanes x one 16-bit word (2 bits per state, 8 states per lane)


class Alignment(NamedTuple):
    """One clip: frame_pos [T] int32 (-1 = blank frame), score (log-probability of the best path; -1e30 when the label has no alignment),
    spans = [(symbol, start, end, conf)] in label order: the class of the symbol, its frames [start, end) and its confidence."""
    frame_pos: np.ndarray
    score: float
    spans: List[Tuple[int, int, int, float]]


def _align_one(x: np.ndarray, y: np.ndarray, blank: int):
    T, C = x.shape
    L = y.shape[0]
    frame_pos = np.full(T, -1, np.int32)
    start, end = np.full(L, -1, np.int32), np.full(L, -1, np.int32)
    conf = np.zeros(L, np.float64)
    isb = np.nonzero(y == blank)[0]
    n = int(isb[0]) if isb.size else L
    lab = y[:n]
    rep = int((lab[1:] == lab[:-1]).sum())
    if ((lab < 0) | (lab >= C)).any() or T < n + rep:
        return frame_pos, start, end, conf, np.float64(INFEASIBLE_SCORE)
    S = 2 * n + 1
    ext = np.full(S, blank, np.int64)
    ext[1::2] = lab
    skip = np.zeros(S, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    E = x[:, ext].astype(np.float64)                           # [T, S]
    dead1, dead2 = np.full(1, -np.inf), np.full(2, -np.inf)
    v = np.full(S, -np.inf)
    v[:min(S, 2)] = E[0, :min(S, 2)]
    bp = np.zeros((T, S), np.int8)
    for t in range(1, T):
        p1 = np.concatenate([dead1, v[:-1]])
        p2 = np.where(skip, np.concatenate([dead2, v[:-2]])[:S], -np.inf)
        best, b = v, bp[t]
        m = p1 > best
        best = np.where(m, p1, best)
        b[m] = 1
        m = p2 > best
        best = np.where(m, p2, best)
        b[m] = 2
        v = best + E[t]
    s = S - 1
    if n > 0 and v[S - 2] > v[S - 1]:
        s = S - 2
    V = v[s]
    path = np.empty(T, np.int64)
    for t in range(T - 1, -1, -1):
        path[t] = s
        s = max(s - int(bp[t, s]), 0)
    frame_pos = np.where(path & 1, path >> 1, -1).astype(np.int32)
    x64 = x.astype(np.float64)
    m = x64.max(axis=1)
    e = np.exp(x64 - m[:, None])
    den = e.sum(axis=1)
    score = (V - m.sum()) - np.log(den).sum()
    emit = np.nonzero(frame_pos >= 0)[0]
    sym = frame_pos[emit]
    first = np.concatenate([[True], sym[1:] != sym[:-1]]) if emit.size else np.zeros(0, bool)
    last = np.concatenate([sym[1:] != sym[:-1], [True]]) if emit.size else np.zeros(0, bool)
    start[sym[first]] = emit[first]
    end[sym[last]] = emit[last] + 1
    p = e[emit, lab[sym]] / den[emit]
    tot = np.zeros(L, np.float64)
    np.add.at(tot, sym, p)
    conf[:n] = tot[:n] / np.maximum(end[:n] - start[:n], 1)
    return frame_pos, start, end, conf, np.float64(score)


def viterbi_align(logits, labels, blank: int):
    """The host reference (module docstring): logits [T, C] with labels [L], or [B, T, C] with [B, L] -> (frame_pos, start, end, conf,
    score), with a leading batch axis for a batch.  frame_pos, start and end are int32; conf and score are kept in fp64 (the device rounds
    them to fp32).  Vectorised over the lattice states, a loop over the frames."""
    x = np.asarray(logits, dtype=np.float32)
    y = np.asarray(labels, dtype=np.int64)
    if x.ndim not in (2, 3) or y.ndim != x.ndim - 1:
        raise ValueError(f"logits [T, C] with labels [L], or [B, T, C] with [B, L]; got {x.shape} and {y.shape}")
    if not 0 <= blank < x.shape[-1]:
        raise ValueError(f"blank {blank} outside 0..{x.shape[-1] - 1}")
    if x.ndim == 2:
        return _align_one(x, y, int(blank))
    if y.shape[0] != x.shape[0]:
        raise ValueError(f"{x.shape[0]} clips but {y.shape[0]} label rows")
    out = [_align_one(x[b], y[b], int(blank)) for b in range(x.shape[0])]
    B, T, L = x.shape[0], x.shape[1], y.shape[1]
    shapes = ((B, T), (B, L), (B, L), (B, L), (B,))
    dtypes = (np.int32, np.int32, np.int32, np.float64, np.float64)
    return tuple(np.array([o[k] for o in out], dtype=dt).reshape(sh) for k, (sh, dt) in enumerate(zip(shapes, dtypes)))


def to_alignments(labels, frame_pos, start, end, conf, score) -> List[Alignment]:
    """The labels [B, L] and the five batched arrays -> one Alignment per clip; a span's symbol is the label's class, spans in label order."""
    out = []
    for b in range(len(score)):
        spans = [(int(labels[b, i]), int(start[b, i]), int(end[b, i]), float(conf[b, i])) for i in range(start.shape[1]) if start[b, i] >= 0]
        out.append(Alignment(np.asarray(frame_pos[b], np.int32), float(score[b]), spans))
    return out


# ---------------------------------------------------------------------------------------------------- device side (ishara_ctc_align)
def check_device_args(C: int, T: int, L: int, blank: int) -> None:
    """The kernel's limits (include/ishara_hip.h), checked before any launch or capture."""
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"C={C} outside 2..{MAX_CLASSES} (one lane per class)")
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"T={T} outside 1..{MAX_FRAMES}")
    if not 1 <= L <= MAX_LABEL:
        raise ValueError(f"L={L} outside 1..{MAX_LABEL}")
    if not 0 <= blank < C:
        raise ValueError(f"blank {blank} outside 0..{C - 1}")


def workspace_bytes(lib, B: int, T: int, L: int) -> int:
    n = int(lib.ishara_ctc_align_workspace_bytes(B, T, L))
    if n < 0:
        raise ValueError(f"no alignment workspace for B={B} T={T} L={L}")
    return n


def launch(lib, logits, labels, B: int, T: int, C: int, L: int, blank: int, ws, frame_pos, start, end, conf, score, stream,
           frame_len=None, ex: bool = False) -> None:
    """One ishara_ctc_align launch on `stream` (graph-capturable).  With frame_len (int32 [B] on the device: the frames of each clip) or
    ex, the launch is ishara_ctc_align_ex."""
    from . import _lib
    if frame_len is not None or ex:
        _lib.check(lib.ishara_ctc_align_ex(_lib.ptr(logits), _lib.ptr(labels), B, T, C, L, blank, _lib.ptr(ws), _lib.ptr(frame_pos), _lib.ptr(start),
                                           _lib.ptr(end), _lib.ptr(conf), _lib.ptr(score), _lib.ptr(frame_len), stream), "ishara_ctc_align_ex")
        return
    _lib.check(lib.ishara_ctc_align(_lib.ptr(logits), _lib.ptr(labels), B, T, C, L, blank, _lib.ptr(ws), _lib.ptr(frame_pos), _lib.ptr(start),
                                    _lib.ptr(end), _lib.ptr(conf), _lib.ptr(score), stream), "ishara_ctc_align")


# `ishara_amd.ctc_align` names this module (the semantics, the host reference, launch) and is also the call of the public surface,
# `ishara_amd.ctc_align(logits, labels, lengths)`, next to ctc_loss / ctc_greedy_decode / ctc_beam_decode: the module is callable.
class _Module(type(np)):
    def __call__(self, *args, **kw):
        from .ctc import ctc_align
        return ctc_align(*args, **kw)


import sys as _sys  # noqa: E402

_sys.modules[__name__].__class__ = _Module
