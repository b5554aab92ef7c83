"""CTC prefix beam search with an optional character-bigram LM: the host reference of `ishara_ctc_beam_decode` (csrc/ctc_beam.hip).

`decode_phrase` (conv-hybrid-model.ipynb c8:4-12, `ishara_greedy_decode`) keeps the best path only.  A prefix beam search (Hannun et al.
2014, "First-pass large vocabulary continuous speech recognition using bi-directional recurrent DNNs") sums over the alignments of each
labeling prefix instead, and can add a character language model by shallow fusion.  The semantics below are implemented exactly by both
this module (numpy, fp64, prefixes compared as tuples) and the kernel (fp32, one workgroup per clip); see DESIGN.md for the kernel layout.

Inputs per clip: logits x [T, C], blank b (callers pass C - 1), beam width W, nbest <= W, an optional table lm [C, C] of natural-log
probabilities (row r = previous character, row b = start of phrase; column c != b = next character, column b = end of phrase), and the
weights alpha (LM) and beta (bonus per emitted character).  The LM term is used only when lm is given and alpha != 0.

  lp[t] = log_softmax(x[t]).  A beam is (prefix, pb, pnb): the log-probabilities of the prefix's alignments up to frame t that end in a
  blank / in a non-blank.  Start: {"": pb = 0, pnb = -inf}.  Per frame, from the beams in rank order:
    same prefix    pb' = (pb (+) pnb) + lp[b],   pnb' = pnb + lp[last]   (-inf for the empty prefix)
    extension c    pnb' = (c == last ? pb : pb (+) pnb) + lp[c]          for every c != b
  (+) is log-add-exp (-inf (+) -inf = -inf).  A candidate whose score is -inf (no alignment reaches it) is dropped.  An extension whose prefix equals a surviving beam is not a candidate of its own: it is merged
  into that beam's pnb' as pnb' = pnb' (+) extension (the beam's own term first).  Ranking key of a candidate:
    score = (pb' (+) pnb') + alpha * LMsum(prefix) + beta * len(prefix),   LMsum = sum of lm[prev][c] over the prefix, from row b.
  The W best candidates survive, in one total order: higher score first; then the same-prefix candidate before extensions; then the lower
  source-beam rank; then the lower class index.  After the last frame every beam gets alpha * lm[last][b] (end of phrase); the beams are
  ranked again by (higher final score, lower beam rank) and the first nbest are returned.

lm may also be an LMAutomaton or a CharNGramLM (ctc_lm.py; the device side is `ishara_ctc_beam_decode_lm`): every beam then carries an LM
state from `start`; an extension by c adds alpha * logp[state][c] and moves to next[state][c], and the final term is
alpha * logp[state][b].  The table is the automaton whose state is the last character, and everything else above is unchanged.

Unlike `decode_phrase`, which never emits the final run of frames (the reference's quirk, kept in the greedy path), the beam search uses
every frame: on logits that end in blank frames the two agree on confident inputs.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

NEG_INF = -math.inf
MAX_CLASSES = 64          # kernel limits (one lane per class, one wavefront list of 32 per beam group, T frames per workgroup loop)
MAX_BEAM = 32
MAX_FRAMES = 4096


def _lse(a, b):
    """log(e^a + e^b) elementwise, -inf (+) -inf = -inf (no NaN).  The kernel's formula: max + log1p(exp(-|a - b|))."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(a - b)
        r = m + np.log1p(np.exp(-d))
    return np.where(m == NEG_INF, NEG_INF, r)


def _gap(hi: float, lo: float) -> float:
    d = float(hi) - float(lo) if hi > lo else 0.0          # -inf vs -inf is a tie
    return d


def log_softmax(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _lm_table(lm, C: int) -> Optional[np.ndarray]:
    if lm is None:
        return None
    t = np.asarray(lm, dtype=np.float64)
    if t.shape != (C, C):
        raise ValueError(f"lm must be [{C}, {C}], got {t.shape}")
    return t


def _lm_rows(lm, C: int, b: int):
    """(logp [S, C] fp64, next [S, C] or None, start): an LMAutomaton or a CharNGramLM (ctc_lm.py) as they are, a table as the automaton
    whose state is the last character (next = None stands for next[s, c] = c; start = blank).  (None, None, b) without an LM."""
    from .ctc_lm import as_automaton
    aut = as_automaton(lm)
    if aut is None:
        return _lm_table(lm, C), None, b
    if aut.num_classes != C:
        raise ValueError(f"the lm has {aut.num_classes} classes, the logits {C}")
    return aut.logp.astype(np.float64), aut.next, aut.start


def prefix_beam_search(logits, beam_width: int, nbest: int = 1, lm=None, alpha: float = 0.0, beta: float = 0.0,
                       blank: Optional[int] = None, return_margin: bool = False):
    """One clip: logits [T, C] -> list of (indices int64, score) in rank order, at most nbest entries (fewer when fewer distinct
    hypotheses exist).  Any beam_width >= 1 is accepted here (the kernel takes 1..32).

    With return_margin, returns (hyps, margin): the smallest score gap over the clip between the W-th and (W+1)-th candidate of every
    frame, and between consecutive entries among the first nbest + 1 final hypotheses.  Where it exceeds the device's rounding, the
    kernel must return the same n-best list."""
    x = np.asarray(logits, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError(f"logits must be [T, C], got {x.shape}")
    T, C = x.shape
    b = C - 1 if blank is None else int(blank)
    if not 0 <= b < C:
        raise ValueError(f"blank {b} outside 0..{C - 1}")
    if beam_width < 1 or nbest < 1 or nbest > beam_width:
        raise ValueError(f"need 1 <= nbest ({nbest}) <= beam_width ({beam_width})")
    table, nxt, start = _lm_rows(lm, C, b)                  # every beam carries its LM state; with a table that is its last character
    use_lm = table is not None and alpha != 0.0
    lp = log_softmax(x)
    cls = np.arange(C)
    margin = math.inf

    prefixes: List[Tuple[int, ...]] = [()]
    pb, pnb = np.zeros(1), np.full(1, NEG_INF)
    lmsum, ln, last = np.zeros(1), np.zeros(1, np.int64), np.full(1, -1, np.int64)
    state = np.full(1, start, np.int64)
    for t in range(T):
        nb = len(prefixes)
        lpt = lp[t]
        tot = _lse(pb, pnb)
        s_pb = tot + lpt[b]
        s_pnb = np.where(last >= 0, pnb + lpt[np.maximum(last, 0)], NEG_INF)
        merged = np.zeros((nb, C), dtype=bool)
        index = {p: r for r, p in enumerate(prefixes)}
        for j in range(nb):
            if ln[j] == 0:
                continue
            i = index.get(prefixes[j][:-1])
            if i is None:
                continue
            c = int(last[j])
            ext = (pb[i] if last[i] == c else tot[i]) + lpt[c]
            s_pnb[j] = _lse(s_pnb[j], ext)
            merged[i, c] = True
        bonus = (alpha * lmsum if use_lm else 0.0) + beta * ln
        s_score = _lse(s_pb, s_pnb) + bonus
        e_pnb = np.where(cls[None, :] == last[:, None], pb[:, None], tot[:, None]) + lpt[None, :]
        e_lm = lmsum[:, None] + table[state] if use_lm else np.zeros((nb, C))
        e_score = e_pnb + ((alpha * e_lm) if use_lm else 0.0) + beta * (ln[:, None] + 1)
        ok = ~merged & (e_score > NEG_INF)
        ok[:, b] = False
        ei, ec = np.nonzero(ok)
        si = np.nonzero(s_score > NEG_INF)[0]
        score = np.concatenate([s_score[si], e_score[ei, ec]])
        kind = np.concatenate([np.zeros(si.size, np.int64), np.ones(ei.size, np.int64)])
        src = np.concatenate([si, ei])
        cc = np.concatenate([np.zeros(si.size, np.int64), ec])
        order = np.lexsort((cc, src, kind, -score))
        if order.size > beam_width:
            margin = min(margin, _gap(score[order[beam_width - 1]], score[order[beam_width]]))
        keep = order[:beam_width]
        n_pref, n_pb, n_pnb, n_lm, n_ln, n_last, n_state = [], [], [], [], [], [], []
        for k in keep:
            s = int(src[k])
            if kind[k] == 0:
                n_pref.append(prefixes[s]); n_pb.append(s_pb[s]); n_pnb.append(s_pnb[s])
                n_lm.append(lmsum[s]); n_ln.append(ln[s]); n_last.append(last[s]); n_state.append(state[s])
            else:
                c = int(cc[k])
                n_pref.append(prefixes[s] + (c,)); n_pb.append(NEG_INF); n_pnb.append(e_pnb[s, c])
                n_lm.append(e_lm[s, c] if use_lm else 0.0); n_ln.append(ln[s] + 1); n_last.append(c)
                n_state.append(c if nxt is None else nxt[state[s], c])
        prefixes = n_pref
        pb, pnb = np.array(n_pb, np.float64), np.array(n_pnb, np.float64)
        lmsum, ln, last = np.array(n_lm, np.float64), np.array(n_ln, np.int64), np.array(n_last, np.int64)
        state = np.array(n_state, np.int64)

    final = _lse(pb, pnb) + ((alpha * lmsum if use_lm else 0.0) + beta * ln)
    if use_lm:
        final = final + alpha * table[state, b]
    order = np.lexsort((np.arange(final.size), -final))
    for k in range(min(nbest, order.size - 1)):
        margin = min(margin, _gap(final[order[k]], final[order[k + 1]]))
    hyps = [(np.array(prefixes[k], dtype=np.int64), float(final[k])) for k in order[:nbest]]
    return (hyps, margin) if return_margin else hyps


class CharBigramLM:
    """A character bigram in natural-log probabilities, table [C, C] float32: row r = previous character (row `blank` = start of
    phrase), column c = next character (column `blank` = end of phrase).  Every row sums to 1 in probability.  `np.asarray(lm)` is the
    table, so an instance goes wherever an lm table does."""

    def __init__(self, table, blank: Optional[int] = None):
        t = np.asarray(table, dtype=np.float32)
        if t.ndim != 2 or t.shape[0] != t.shape[1]:
            raise ValueError(f"an LM table is [C, C], got {t.shape}")
        self.table = t
        self.blank = t.shape[0] - 1 if blank is None else int(blank)

    def __array__(self, dtype=None, copy=None):
        return self.table if dtype is None else self.table.astype(dtype)

    @classmethod
    def fit(cls, phrases: Sequence[Union[str, Sequence[int]]], char_to_num: Optional[Dict[str, int]] = None, num_classes: int = 60,
            smoothing: float = 0.1, blank: Optional[int] = None) -> "CharBigramLM":
        """Add-`smoothing` estimate from phrases (strings through char_to_num, or index sequences in [0, num_classes) without the
        blank).  Each phrase contributes BOS -> c0, c_k -> c_k+1 and c_last -> EOS."""
        C = int(num_classes)
        b = C - 1 if blank is None else int(blank)
        if smoothing <= 0:
            raise ValueError("smoothing must be > 0 (a zero count would give log 0)")
        counts = np.zeros((C, C), dtype=np.float64)
        for p in phrases:
            if isinstance(p, str):
                if char_to_num is None:
                    raise ValueError("string phrases need char_to_num")
                seq = [char_to_num[ch] for ch in p]
            else:
                seq = [int(v) for v in p]
            if any(v < 0 or v >= C or v == b for v in seq):
                raise ValueError(f"phrase {p!r}: indices must lie in [0, {C}) and differ from the blank {b}")
            prev = b
            for v in seq:
                counts[prev, v] += 1
                prev = v
            counts[prev, b] += 1
        counts += smoothing
        table = np.log(counts / counts.sum(axis=1, keepdims=True))
        return cls(table.astype(np.float32), b)

    def save(self, path: str) -> str:
        np.save(path, self.table)
        return path if path.endswith(".npy") else path + ".npy"

    @classmethod
    def load(cls, path: str, blank: Optional[int] = None) -> "CharBigramLM":
        return cls(np.load(path), blank)

    def sample(self, rng: np.random.Generator, max_len: int) -> List[int]:
        """One phrase drawn from the bigram (stops at EOS or max_len)."""
        p = np.exp(self.table.astype(np.float64))
        p /= p.sum(axis=1, keepdims=True)
        out, prev = [], self.blank
        while len(out) < max_len:
            c = int(rng.choice(p.shape[1], p=p[prev]))
            if c == self.blank:
                break
            out.append(c)
            prev = c
        return out


# ---------------------------------------------------------------------------------------------------- device side (ishara_ctc_beam_decode)
def check_device_args(C: int, T: int, beam_width: int, nbest: int) -> None:
    """The kernel's limits (include/ishara_hip.h), checked before any launch or capture."""
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"C={C} outside 2..{MAX_CLASSES} (one lane per class)")
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"T={T} outside 1..{MAX_FRAMES}")
    if not 1 <= beam_width <= MAX_BEAM:
        raise ValueError(f"beam_width {beam_width} outside 1..{MAX_BEAM}")
    if not 1 <= nbest <= beam_width:
        raise ValueError(f"nbest {nbest} outside 1..beam_width={beam_width}")


def lm_to_device(lm, C: int, device):
    """The LM table as a contiguous fp32 [C, C] device tensor (None stays None); a CharNGramLM or an LMAutomaton as the DeviceAutomaton
    of ctc_lm.py, which `launch` sends to ishara_ctc_beam_decode_lm."""
    import torch
    from . import ctc_lm
    if lm is None:
        return None
    aut = ctc_lm.as_automaton(lm)
    if aut is not None:
        return ctc_lm.DeviceAutomaton(aut, C, device)
    t = np.asarray(lm, dtype=np.float32)
    if t.shape != (C, C):
        raise ValueError(f"lm must be [{C}, {C}], got {t.shape}")
    return torch.from_numpy(np.ascontiguousarray(t)).to(device)


def workspace_bytes(lib, B: int, T: int, C: int, beam_width: int) -> int:
    n = int(lib.ishara_ctc_beam_workspace_bytes(B, T, C, beam_width))
    if n < 0:
        raise ValueError(f"no beam workspace for B={B} T={T} W={beam_width}")
    return n


def launch(lib, logits, B: int, T: int, C: int, beam_width: int, nbest: int, lm_dev, alpha: float, beta: float, ws, out_idx, out_len,
           out_score, stream, frame_len=None, ex: bool = False) -> None:
    """One ishara_ctc_beam_decode launch on `stream` (graph-capturable); blank = C - 1 as for the greedy decoder.  With frame_len (int32
    [B] on the device: the frames of each clip) or ex, the launch is ishara_ctc_beam_decode_ex.  An lm_dev that is a DeviceAutomaton
    goes to ishara_ctc_beam_decode_lm, with or without frame_len."""
    import ctypes as C_
    from . import _lib
    from .ctc_lm import entry_point
    if entry_point(lm_dev) == "ishara_ctc_beam_decode_lm":
        _lib.check(lib.ishara_ctc_beam_decode_lm(_lib.ptr(logits), B, T, C, C - 1, beam_width, nbest, _lib.ptr(lm_dev.logp), _lib.ptr(lm_dev.next),
                                                 lm_dev.S, lm_dev.start, C_.c_float(alpha), C_.c_float(beta), _lib.ptr(ws), _lib.ptr(out_idx),
                                                 _lib.ptr(out_len), _lib.ptr(out_score), _lib.ptr(frame_len), stream),
                   "ishara_ctc_beam_decode_lm")
        return
    if frame_len is not None or ex:
        _lib.check(lib.ishara_ctc_beam_decode_ex(_lib.ptr(logits), B, T, C, C - 1, beam_width, nbest,
                                                 _lib.ptr(lm_dev) if lm_dev is not None else None, C_.c_float(alpha), C_.c_float(beta),
                                                 _lib.ptr(ws), _lib.ptr(out_idx), _lib.ptr(out_len), _lib.ptr(out_score), _lib.ptr(frame_len), stream),
                   "ishara_ctc_beam_decode_ex")
        return
    _lib.check(lib.ishara_ctc_beam_decode(_lib.ptr(logits), B, T, C, C - 1, beam_width, nbest,
                                          _lib.ptr(lm_dev) if lm_dev is not None else None, C_.c_float(alpha), C_.c_float(beta),
                                          _lib.ptr(ws), _lib.ptr(out_idx), _lib.ptr(out_len), _lib.ptr(out_score), stream),
               "ishara_ctc_beam_decode")
