"""Second-pass n-best rescoring: the host references and the device entries of `ishara_ctc_score_nbest` (csrc/ctc_score.hip) and
`ishara_nbest_rescore` / `ishara_nbest_rescore_p` (csrc/nbest_rescore.hip) and `ishara_rescore_sweep` (csrc/rescore_sweep.hip); contracts in
include/ishara_hip.h.

Every other decoder of this package ranks a hypothesis by the score the beam search attached to it.  That score sums only the alignments
that survived the beam (a lower bound on log P(h | x) whose slack differs from hypothesis to hypothesis), exists only under the model that
found the hypothesis, and carries the LM of the search.  The second pass removes the three limits:

  score     logp_m[b, n] = log P_m(h_n | x_b): the full CTC forward sum of every hypothesis under every model (each model its own T)
  combine   s = sum_m w_m logp_m + alpha * LM(h) + beta * len(h), the LM a CharNGramLM / LMAutomaton / bigram table that the search need
            not have used (search small or without an LM, rescore with a large one)
  dedupe    a string found twice (by two models of a pooled list) keeps its first slot; the later one dies
  rerank    live slots by descending s, ties to the lower slot; a -inf score stays live and ranks last among the numbers
  posterior p = exp((s - s_max) / temperature) / sum over the live slots with a finite score: a confidence, and the weights= of mbr_select

  ctc_logp_reference, rescore_reference    one clip in numpy (fp64 forward algorithm; the device's float32 score arithmetic)
  ctc_score_nbest, rescore_nbest           device tensors in, device tensors out, on the current stream, nothing waits (params=: the
                                           weights, alpha and beta in one device tensor that a captured graph follows)
  sweep_grid, rescore_sweep, sweep_scores  choosing w_m / alpha / beta on a held-out set: every row of a parameter grid in ONE launch
                                           (ishara_rescore_sweep: the top slot per row and its edit distance to the target);
                                           rescore_sweep_reference is its definition
  rescore_models                           a pooled list (mbr.pool_nbest) scored under every model and rescored: sequence-level ensembling
                                           for models that the frame-level fusion (ensemble.py) cannot combine
  Model.rescore_decode                     beam search, exact scores, rescoring, top-1 or the MBR choice

Wired: TFLiteModel / BatchedTFLiteModel / EnsembleTFLiteModel(rescore_nbest=, rescore_lm=, rescore_alpha=, rescore_beta=,
rescore_temperature=) capture search, exact scores and ishara_nbest_rescore_p in their graph (the ensemble on its fused rows, M = 1),
set_rescore rewrites the parameters on the device, BatchedTFLiteModel.score_rescore_grid sweeps them with one ishara_rescore_sweep per batch.
Not wired: sequence-level multi-model rescoring (rescore_models) inside a wrapper; streaming (StreamingTFLiteModel refuses the option); the
MBR vote in the sweep (it follows the top-1 choice only).  No accuracy effect on real data is measured anywhere in this repository: there
is no dataset and there are no trained weights.
"""
from __future__ import annotations

import ctypes as C_
import math
from typing import Optional, Sequence

import numpy as np

MAX_NBEST = 64
MAX_FRAMES = 4096
MAX_CLASSES = 64
MAX_MODELS = 8
MAX_HYP_LEN = 255          # the loss kernel's label limit
STATUS_DEAD, STATUS_NO_ALIGNMENT, STATUS_SYMBOL, STATUS_LONG = 1, 2, 4, 8


# ---------------------------------------------------------------------------------------------------- host references
def ctc_logp_reference(logits, hyp: Sequence[int], blank: Optional[int] = None) -> float:
    """log P(hyp | logits) of one clip by the CTC forward algorithm in fp64: logits [T, C] (log_softmax is taken here), hyp a sequence of
    classes other than blank (empty: the all-blank path), blank defaults to C - 1.  -inf when no alignment exists (T < len + repeats)."""
    x = np.asarray(logits, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 1:
        raise ValueError(f"logits must be [T >= 1, C], got {x.shape}")
    T, Cn = x.shape
    b = Cn - 1 if blank is None else int(blank)
    if not 0 <= b < Cn:
        raise ValueError(f"blank {b} outside 0..{Cn - 1}")
    h = [int(v) for v in hyp]
    if any(v < 0 or v >= Cn or v == b for v in h):
        raise ValueError(f"hypothesis symbols must lie in [0, {Cn}) and differ from the blank {b}")
    m = x.max(axis=1, keepdims=True)
    lp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True)))
    ext = np.full(2 * len(h) + 1, b, np.int64)
    ext[1::2] = h
    S = ext.shape[0]
    skip = np.zeros(S, bool)                                 # s-2 -> s
    skip[2:] = (ext[2:] != b) & (ext[2:] != ext[:-2])
    a = np.full(S, -np.inf)
    a[0] = lp[0, b]
    if S > 1:
        a[1] = lp[0, ext[1]]
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            a1 = np.concatenate([[-np.inf], a[:-1]])
            a2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], a[:-2]]), -np.inf)
            a = np.logaddexp(np.logaddexp(a, a1), a2) + lp[t, ext]
    return float(np.logaddexp(a[S - 1], a[S - 2]) if S > 1 else a[0])


def _lm_host(lm, blank: Optional[int]):
    """the LMAutomaton of an lm= argument, or None; a bigram table goes through LMAutomaton.from_bigram"""
    from .ctc_lm import LMAutomaton, as_automaton
    if lm is None:
        return None
    aut = as_automaton(lm)
    if aut is None:
        aut = LMAutomaton.from_bigram(lm, blank)
    return aut


def rescore_reference(hyps, logps, weights=None, lm=None, alpha: float = 0.0, beta: float = 0.0, inv_temp: float = 1.0,
                      blank: Optional[int] = None):
    """One clip on the host.  hyps: N entries, each a sequence of integers or None for a dead slot; logps [M, N]: the per-model scores
    (float32 values, e.g. the device's own logp); weights [M] (default all 1); lm: a CharNGramLM, an LMAutomaton or a [C, C] table; blank:
    the LM's end-of-phrase column (default C - 1).  The score is computed in float32 in the device's order (module docstring of
    csrc/nbest_rescore.hip) and equals its bits; the posterior is fp64 from those float32 scores.
    Returns (order, out_score float32 [N], live [N] bool, posterior float64 [N]) by OUTPUT slot: order[r] = the input slot, live[r] False
    for dead or merged slots (out_score -inf there)."""
    f32 = np.float32
    N = len(hyps)
    if N < 1:
        raise ValueError("an n-best list has at least one slot")
    lp = np.asarray(logps, f32)
    if lp.ndim != 2 or lp.shape[1] != N:
        raise ValueError(f"logps must be [M, {N}], got {lp.shape}")
    M = lp.shape[0]
    w = np.ones(M, f32) if weights is None else np.asarray(weights, f32)
    if w.shape != (M,):
        raise ValueError(f"weights must be {M} numbers, got shape {w.shape}")
    aut = _lm_host(lm, blank)
    seqs = [None if h is None else tuple(int(v) for v in h) for h in hyps]
    live = np.array([s is not None for s in seqs])
    seen = {}
    for n, s in enumerate(seqs):                             # the earlier slot stays
        if s is None:
            continue
        if s in seen:
            live[n] = False
        else:
            seen[s] = n
    a32, b32 = f32(alpha), f32(beta)
    score = np.full(N, -np.inf, f32)
    with np.errstate(all="ignore"):
        for n in range(N):
            if not live[n]:
                continue
            s = f32(0.0)
            for m in range(M):
                if w[m] > 0:
                    s = f32(s + f32(w[m] * lp[m, n]))
            if aut is not None:
                Cn = aut.num_classes
                eos = Cn - 1 if blank is None else int(blank)
                if any(c < 0 or c >= Cn for c in seqs[n]):
                    s = f32(-np.inf)
                else:
                    l, state = f32(0.0), aut.start
                    for c in seqs[n]:
                        l = f32(l + aut.logp[state, c])
                        state = int(aut.next[state, c])
                        state = state if 0 <= state < aut.num_states else 0
                    l = f32(l + aut.logp[state, eos])
                    s = f32(s + f32(a32 * l))
            s = f32(s + f32(b32 * f32(len(seqs[n]))))
            score[n] = s
    cls = np.where(~live, 2, np.where(np.isnan(score), 1, 0))
    key = np.where(cls == 0, -np.where(cls == 0, score, f32(0.0)).astype(np.float64), 0.0)
    order = np.lexsort((np.arange(N), key, cls))            # class, then descending score, then the lower slot
    out_score = np.where(live[order], score[order], f32(-np.inf)).astype(f32)
    live_o = live[order]
    fin = live_o & np.isfinite(out_score)
    post = np.zeros(N, np.float64)
    if fin.any():
        s64 = out_score.astype(np.float64)
        e = np.exp((s64[fin] - s64[fin].max()) * float(f32(inv_temp)))
        post[fin] = e / e.sum()
    return order.astype(np.int64), out_score, live_o, post


# ---------------------------------------------------------------------------------------------------- device side
def _cuda(t, dtype, shape, what: str):
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a torch tensor on the GPU, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what} must be on the GPU (the rescoring kernels have no CPU path; rescore.py holds the host references)")
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be {list(shape)}, got {list(t.shape)}")
    return t.contiguous()


def _nbest(hyp_idx, hyp_len):
    import torch
    hyp_idx = _cuda(hyp_idx, torch.int32, None, "hyp_idx")
    if hyp_idx.ndim != 3:
        raise ValueError(f"hyp_idx must be [B, N, Th], got {tuple(hyp_idx.shape)}")
    B, N, Th = hyp_idx.shape
    if not 1 <= N <= MAX_NBEST:
        raise ValueError(f"N={N} hypotheses per clip outside 1..{MAX_NBEST} (one lane per hypothesis)")
    if not 1 <= Th <= MAX_FRAMES:
        raise ValueError(f"Th={Th} outside 1..{MAX_FRAMES}")
    hyp_len = _cuda(hyp_len, torch.int32, (B, N), "hyp_len")
    if hyp_len.device != hyp_idx.device:
        raise ValueError("hyp_idx and hyp_len must be on one device")
    return hyp_idx, hyp_len, B, N, Th


def ctc_score_nbest(logits, hyp_idx, hyp_len, lengths=None, blank: Optional[int] = None, return_status: bool = False):
    """log P(h | x) of every hypothesis of every clip under one model, on the device (ishara_ctc_score_nbest).  logits fp32 [B, T, C];
    hyp_idx int32 [B, N, Th] / hyp_len int32 [B, N] as ctc.ctc_beam_nbest_device and mbr.pool_nbest give them (Th need not be T); lengths:
    the clips' frame counts (a list, an array or a tensor; None: T each); blank defaults to C - 1.  Runs on the current stream, nothing
    waits.  Returns logp fp32 [B, N] (-inf for a dead slot, a hypothesis without an alignment, a bad symbol, a length above min(Th, 255));
    with return_status also status int32 [B, N] (STATUS_* bits, 0 for a scored slot)."""
    import torch
    from . import _lib, ctc
    hyp_idx, hyp_len, B, N, Th = _nbest(hyp_idx, hyp_len)
    x = _cuda(logits, torch.float32, None, "logits")
    if x.ndim != 3 or x.shape[0] != B:
        raise ValueError(f"logits must be [B={B}, T, C], got {tuple(x.shape)}")
    if x.device != hyp_idx.device:
        raise ValueError("logits and hyp_idx must be on one device")
    _, T, Cn = x.shape
    if not 2 <= Cn <= MAX_CLASSES:
        raise ValueError(f"C={Cn} outside 2..{MAX_CLASSES}")
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"T={T} outside 1..{MAX_FRAMES}")
    blank = Cn - 1 if blank is None else int(blank)
    if not 0 <= blank < Cn:
        raise ValueError(f"blank {blank} outside 0..{Cn - 1}")
    fl = None if lengths is None else ctc._lengths(lengths, B, T, 1, "lengths", x.device)
    logp = torch.empty((B, N), dtype=torch.float32, device=x.device)
    status = torch.empty((B, N), dtype=torch.int32, device=x.device) if return_status else None
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ishara_ctc_score_nbest(_lib.ptr(x), B, T, Cn, blank, _lib.ptr(hyp_idx), _lib.ptr(hyp_len), N, Th, _lib.ptr(fl),
                                                      _lib.ptr(logp), _lib.ptr(status), _lib.stream()), "ishara_ctc_score_nbest")
    return (logp, status) if return_status else logp


def pointer_array(tensors):
    """the host array of device pointers ishara_nbest_rescore takes"""
    return (C_.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def lm_to_device(lm, device, blank: Optional[int] = None):
    """lm= as a ctc_lm.DeviceAutomaton on `device` (None stays None; a DeviceAutomaton is handed on)"""
    from .ctc_lm import DeviceAutomaton
    if lm is None or isinstance(lm, DeviceAutomaton):
        return lm
    aut = _lm_host(lm, blank)
    return DeviceAutomaton(aut, aut.num_classes, device)


def launch(lib, hyp_idx, hyp_len, B: int, N: int, Th: int, ptrs, M: int, weights, lm_dev, blank: int, alpha: float, beta: float, inv_temp,
           out_idx, out_len, out_score, posterior, perm, stream) -> None:
    """One ishara_nbest_rescore launch on `stream` (graph-capturable).  ptrs: pointer_array of the M logp tensors; lm_dev: a DeviceAutomaton or None."""
    from . import _lib
    Cn = int(lm_dev.logp.shape[1]) if lm_dev is not None else 0
    _lib.check(lib.ishara_nbest_rescore(_lib.ptr(hyp_idx), _lib.ptr(hyp_len), B, N, Th, ptrs, M, _lib.ptr(weights),
                                        _lib.ptr(lm_dev.logp) if lm_dev is not None else None, _lib.ptr(lm_dev.next) if lm_dev is not None else None,
                                        lm_dev.S if lm_dev is not None else 0, lm_dev.start if lm_dev is not None else 0, Cn, blank,
                                        C_.c_float(alpha), C_.c_float(beta), _lib.ptr(inv_temp), _lib.ptr(out_idx), _lib.ptr(out_len),
                                        _lib.ptr(out_score), _lib.ptr(posterior), _lib.ptr(perm), stream), "ishara_nbest_rescore")


def launch_p(lib, hyp_idx, hyp_len, B: int, N: int, Th: int, ptrs, M: int, params, lm_dev, blank: int, inv_temp, out_idx, out_len, out_score,
             posterior, perm, stream) -> None:
    """One ishara_nbest_rescore_p launch on `stream` (graph-capturable): launch() with (weights, alpha, beta) in the device tensor params [M + 2]."""
    from . import _lib
    Cn = int(lm_dev.logp.shape[1]) if lm_dev is not None else 0
    _lib.check(lib.ishara_nbest_rescore_p(_lib.ptr(hyp_idx), _lib.ptr(hyp_len), B, N, Th, ptrs, M, _lib.ptr(params),
                                          _lib.ptr(lm_dev.logp) if lm_dev is not None else None, _lib.ptr(lm_dev.next) if lm_dev is not None else None,
                                          lm_dev.S if lm_dev is not None else 0, lm_dev.start if lm_dev is not None else 0, Cn, blank,
                                          _lib.ptr(inv_temp), _lib.ptr(out_idx), _lib.ptr(out_len), _lib.ptr(out_score), _lib.ptr(posterior),
                                          _lib.ptr(perm), stream), "ishara_nbest_rescore_p")


def rescore_nbest(hyp_idx, hyp_len, logps, weights=None, lm=None, alpha: float = 0.0, beta: float = 0.0, temperature=1.0,
                  return_details: bool = False, blank: Optional[int] = None, params=None):
    """Combine, dedupe, rerank on the device (ishara_nbest_rescore).  hyp_idx int32 [B, N, Th], hyp_len int32 [B, N]; logps: one fp32
    [B, N] tensor or a sequence of M <= 8 (ctc_score_nbest under each model); weights: None (all 1), M numbers, or an fp32 [M] device
    tensor that is handed on unread; lm: a CharNGramLM, an LMAutomaton, a [C, C] bigram table or a ctc_lm.DeviceAutomaton; blank: the LM's
    end-of-phrase column (default C - 1); temperature: a number > 0, or a one-element fp32 device tensor holding 1 / temperature.  Runs on
    the current stream, nothing waits.  params: an fp32 [M + 2] device tensor (w_0 .. w_{M-1}, alpha, beta) handed on unread to
    ishara_nbest_rescore_p in place of weights / alpha / beta, which must then be left at their defaults.
    Returns (out_idx int32 [B, N, Th], out_len int32 [B, N], out_score fp32 [B, N]) in the new order, the layout mbr.mbr_select reads;
    with return_details also a dict of posterior fp32 [B, N] and perm int32 [B, N] (the input slot of each output slot)."""
    import torch
    from . import _lib, mbr
    hyp_idx, hyp_len, B, N, Th = _nbest(hyp_idx, hyp_len)
    dev = hyp_idx.device
    if isinstance(logps, torch.Tensor):
        logps = [logps]
    logps = [_cuda(t, torch.float32, (B, N), f"logps[{m}]") for m, t in enumerate(logps)]
    M = len(logps)
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f"M={M} models outside 1..{MAX_MODELS}")
    if params is not None:
        if weights is not None or float(alpha) != 0.0 or float(beta) != 0.0:
            raise ValueError("params holds the weights, alpha and beta: give either params or the three")
        params = _cuda(params, torch.float32, (M + 2,), "params")
        w_d = params
    elif isinstance(weights, torch.Tensor):
        w_d = _cuda(weights, torch.float32, (M,), "weights")
    else:
        w = np.ones(M, np.float32) if weights is None else np.asarray(weights, np.float32)
        if w.shape != (M,):
            raise ValueError(f"weights must be {M} numbers (one per model), got shape {w.shape}")
        w_d = torch.from_numpy(w).to(dev)
    if isinstance(temperature, torch.Tensor):
        it_d = _cuda(temperature, torch.float32, (1,), "temperature (a device tensor holds 1 / temperature)")
    else:
        it = mbr.inverse_temperature(temperature)
        it_d = None if it == 1.0 else torch.full((1,), it, dtype=torch.float32, device=dev)
    if not (math.isfinite(float(alpha)) and math.isfinite(float(beta))):
        raise ValueError("alpha and beta must be finite")
    lm_dev = lm_to_device(lm, dev, blank)
    eos = 0
    if lm_dev is not None:
        Cn = int(lm_dev.logp.shape[1])
        eos = Cn - 1 if blank is None else int(blank)
        if not 0 <= eos < Cn:
            raise ValueError(f"blank {eos} outside 0..{Cn - 1}")
    for t, what in [(w_d, "weights"), (it_d, "temperature")] + [(t, f"logps[{m}]") for m, t in enumerate(logps)]:
        if t is not None and t.device != dev:
            raise ValueError(f"hyp_idx and {what} must be on one device")
    out_idx = torch.empty((B, N, Th), dtype=torch.int32, device=dev)
    out_len = torch.empty((B, N), dtype=torch.int32, device=dev)
    out_score = torch.empty((B, N), dtype=torch.float32, device=dev)
    det = None
    if return_details:
        det = dict(posterior=torch.empty((B, N), dtype=torch.float32, device=dev), perm=torch.empty((B, N), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        if params is not None:
            launch_p(_lib.load(), hyp_idx, hyp_len, B, N, Th, pointer_array(logps), M, params, lm_dev, eos, it_d, out_idx, out_len, out_score,
                     det and det["posterior"], det and det["perm"], _lib.stream())
        else:
            launch(_lib.load(), hyp_idx, hyp_len, B, N, Th, pointer_array(logps), M, w_d, lm_dev, eos, float(alpha), float(beta), it_d, out_idx, out_len,
                   out_score, det and det["posterior"], det and det["perm"], _lib.stream())
    return (out_idx, out_len, out_score, det) if return_details else (out_idx, out_len, out_score)


def rescore_models(logits_list, lengths_list, pooled, model_weights=None, lm=None, alpha: float = 0.0, beta: float = 0.0, temperature=1.0,
                   blank: Optional[int] = None, return_details: bool = False):
    """Sequence-level ensembling: the pooled n-best list of mbr.pool_nbest (hyp_idx, hyp_len[, hyp_score]) scored under every model, one
    ctc_score_nbest call per model, each with its own logits [B, T_m, C] and lengths (lengths_list: None, or one entry per model, each None
    or the clips' frame counts), then one rescore_nbest call with model_weights.  Returns what rescore_nbest returns; with return_details the
    dict also holds logps, the per-model score tensors in the INPUT order of the pooled list."""
    logits_list = list(logits_list)
    if not 1 <= len(logits_list) <= MAX_MODELS:
        raise ValueError(f"{len(logits_list)} models outside 1..{MAX_MODELS}")
    lengths_list = [None] * len(logits_list) if lengths_list is None else list(lengths_list)
    if len(lengths_list) != len(logits_list):
        raise ValueError(f"lengths_list has {len(lengths_list)} entries for {len(logits_list)} models")
    hyp_idx, hyp_len = pooled[0], pooled[1]
    logps = [ctc_score_nbest(x, hyp_idx, hyp_len, fl, blank) for x, fl in zip(logits_list, lengths_list)]
    out = rescore_nbest(hyp_idx, hyp_len, logps, model_weights, lm, alpha, beta, temperature, return_details, blank)
    if return_details:
        out[3]["logps"] = logps
    return out



# ---------------------------------------------------------------------------------------------------- the weight sweep
MAX_GRID_ROWS = 65536
MAX_TARGET_LEN = 64        # ishara_edit_distance's: the target is one 64-bit word of the sweep kernel
SWEEP_ROW_TILE = 256       # csrc/rescore_sweep.hip RS_ROWS: the grid rows one workgroup takes (the tests put G on either side of it)
PAD_TOKEN = 59


def sweep_grid(weights, alpha, beta) -> np.ndarray:
    """The cartesian product of candidate values as float32 [G, M + 2], each row a params vector (w_0 .. w_{M-1}, alpha, beta).  weights: a
    list of M candidate lists (one per model); alpha, beta: candidate lists.  Row order: itertools.product(*weights, alpha, beta), i.e. beta
    varies fastest, then alpha, then w_{M-1}, ..., w_0 slowest."""
    import itertools
    cols = [list(np.atleast_1d(np.asarray(c, np.float32))) for c in list(weights) + [alpha, beta]]
    if len(cols) < 3:
        raise ValueError("weights must hold at least one model's candidate list")
    if len(cols) - 2 > MAX_MODELS:
        raise ValueError(f"M={len(cols) - 2} models outside 1..{MAX_MODELS}")
    if any(len(c) == 0 for c in cols):
        raise ValueError("every candidate list needs at least one value")
    G = int(np.prod([len(c) for c in cols]))
    if G > MAX_GRID_ROWS:
        raise ValueError(f"G={G} grid rows outside 1..{MAX_GRID_ROWS}")
    return np.array(list(itertools.product(*cols)), np.float32).reshape(G, len(cols))


def target_symbols(target) -> list:
    """the symbols of a pad-59 target row before the first 59, as ishara_edit_distance reads it"""
    out = []
    for v in np.asarray(target).ravel().tolist():
        if int(v) == PAD_TOKEN:
            break
        out.append(int(v))
    return out


def rescore_sweep_reference(hyps, logps, target, grid, lm=None, blank: Optional[int] = None, fallback: bool = True):
    """One clip on the host: the definition ishara_rescore_sweep is held to.  hyps / logps / lm / blank as rescore_reference; target: the
    clip's symbols (a pad-59 row is cut at the first 59); grid [G, M + 2].  Row g is rescore_reference under (weights, alpha, beta) =
    grid[g]: best[g] = the input slot of its first output slot (-1 when that slot is not live), dist[g] = evaluation.levenshtein of that
    hypothesis (tflite_batch.apply_fallback first when `fallback`; no live slot: the empty string) and the target.
    Returns (best int64 [G], dist int64 [G], tlen, hyp_dist int64 [N]: the distance a slot would report, -1 for dead or merged slots)."""
    from .evaluation import levenshtein
    from .tflite_batch import apply_fallback
    grid = np.asarray(grid, np.float32)
    lp = np.asarray(logps, np.float32)
    if grid.ndim != 2 or lp.ndim != 2 or grid.shape[1] != lp.shape[0] + 2:
        raise ValueError(f"grid must be [G, M + 2] for logps [M, N], got {grid.shape} and {lp.shape}")
    M = lp.shape[0]
    tgt = target_symbols(target)

    def d_of(h):
        a = np.asarray([] if h is None else list(h), np.int64)
        a = apply_fallback(a) if fallback else a
        return int(levenshtein([int(v) for v in a], tgt))

    order0, _, live0, _ = rescore_reference(hyps, lp, np.zeros(M, np.float32), None, 0.0, 0.0, 1.0, blank)      # liveness after the merge
    alive = np.zeros(len(hyps), bool)
    alive[order0[live0]] = True
    hyp_dist = np.array([d_of(h) if alive[n] else -1 for n, h in enumerate(hyps)], np.int64)
    none_d = d_of(None)
    best = np.zeros(grid.shape[0], np.int64)
    dist = np.zeros(grid.shape[0], np.int64)
    for g, row in enumerate(grid):
        order, _, live, _ = rescore_reference(hyps, lp, row[:M], lm, row[M], row[M + 1], 1.0, blank)
        best[g] = int(order[0]) if live[0] else -1
        dist[g] = hyp_dist[best[g]] if live[0] else none_d
    return best, dist, len(tgt), hyp_dist


def sweep_scores(dist, tlen):
    """The c18 mean of every grid row: dist [G, n] (or [G, B] of one batch), tlen [n] -> (means float64 [G], ranking int64 [G]: the rows by
    descending mean, rows of equal means in grid order), each mean through tflite_batch.normalized_scores."""
    from .tflite_batch import normalized_scores
    dist, tlen = np.asarray(dist), np.asarray(tlen)
    if dist.ndim != 2 or tlen.shape != (dist.shape[1],):
        raise ValueError(f"dist must be [G, n] and tlen [n], got {dist.shape} and {tlen.shape}")
    means = np.array([normalized_scores(row, tlen)[0] for row in dist], np.float64)
    return means, np.argsort(-means, kind="stable").astype(np.int64)


def sweep_launch(lib, hyp_idx, hyp_len, B: int, N: int, Th: int, ptrs, M: int, lm_dev, blank: int, targets, L: int, fallback: int, grid, G: int, best,
                 dist, tlen, hyp_dist, lm_score, ws, stream) -> None:
    """One ishara_rescore_sweep launch on `stream` (graph-capturable); arguments as launch()."""
    from . import _lib
    Cn = int(lm_dev.logp.shape[1]) if lm_dev is not None else 0
    _lib.check(lib.ishara_rescore_sweep(_lib.ptr(hyp_idx), _lib.ptr(hyp_len), B, N, Th, ptrs, M, _lib.ptr(lm_dev.logp) if lm_dev is not None else None,
                                        _lib.ptr(lm_dev.next) if lm_dev is not None else None, lm_dev.S if lm_dev is not None else 0,
                                        lm_dev.start if lm_dev is not None else 0, Cn, blank, _lib.ptr(targets), L, fallback, _lib.ptr(grid), G,
                                        _lib.ptr(best), _lib.ptr(dist), _lib.ptr(tlen), _lib.ptr(hyp_dist), _lib.ptr(lm_score), _lib.ptr(ws), stream),
               "ishara_rescore_sweep")


def rescore_sweep(hyp_idx, hyp_len, logps, targets, grid, lm=None, blank: Optional[int] = None, fallback: bool = True, return_details: bool = False):
    """Every row of a parameter grid at once on the device (ishara_rescore_sweep).  hyp_idx int32 [B, N, Th], hyp_len int32 [B, N]; logps:
    one fp32 [B, N] tensor or a sequence of M <= 8; targets int32 [B, L <= 64] padded with 59; grid fp32 [G, M + 2] on the device (sweep_grid
    gives the rows; a numpy array is copied over); lm / blank as rescore_nbest; fallback: the wrapper's len < 3 rule, as ishara_edit_distance
    applies it.  Runs on the current stream, nothing waits.
    Returns (best int32 [G, B], dist int32 [G, B], tlen int32 [B]); with return_details also a dict of hyp_dist int32 [B, N] and lm_score
    fp32 [B, N]."""
    import torch
    from . import _lib
    hyp_idx, hyp_len, B, N, Th = _nbest(hyp_idx, hyp_len)
    dev = hyp_idx.device
    if isinstance(logps, torch.Tensor):
        logps = [logps]
    logps = [_cuda(t, torch.float32, (B, N), f"logps[{m}]") for m, t in enumerate(logps)]
    M = len(logps)
    if not 1 <= M <= MAX_MODELS:
        raise ValueError(f"M={M} models outside 1..{MAX_MODELS}")
    targets = _cuda(targets, torch.int32, None, "targets")
    if targets.ndim != 2 or targets.shape[0] != B or not 1 <= targets.shape[1] <= MAX_TARGET_LEN:
        raise ValueError(f"targets must be [B={B}, L] with 1 <= L <= {MAX_TARGET_LEN}, got {tuple(targets.shape)}")
    if isinstance(grid, np.ndarray):
        grid = torch.from_numpy(np.ascontiguousarray(grid, np.float32)).to(dev)
    grid = _cuda(grid, torch.float32, None, "grid")
    if grid.ndim != 2 or grid.shape[1] != M + 2 or not 1 <= grid.shape[0] <= MAX_GRID_ROWS:
        raise ValueError(f"grid must be [G, M + 2 = {M + 2}] with 1 <= G <= {MAX_GRID_ROWS}, got {tuple(grid.shape)}")
    G = int(grid.shape[0])
    lm_dev = lm_to_device(lm, dev, blank)
    eos = 0
    if lm_dev is not None:
        Cn = int(lm_dev.logp.shape[1])
        eos = Cn - 1 if blank is None else int(blank)
        if not 0 <= eos < Cn:
            raise ValueError(f"blank {eos} outside 0..{Cn - 1}")
    for t, what in [(targets, "targets"), (grid, "grid")] + [(t, f"logps[{m}]") for m, t in enumerate(logps)]:
        if t.device != dev:
            raise ValueError(f"hyp_idx and {what} must be on one device")
    best = torch.empty((G, B), dtype=torch.int32, device=dev)
    dist = torch.empty((G, B), dtype=torch.int32, device=dev)
    tlen = torch.empty((B,), dtype=torch.int32, device=dev)
    det = None
    if return_details:
        det = dict(hyp_dist=torch.empty((B, N), dtype=torch.int32, device=dev), lm_score=torch.empty((B, N), dtype=torch.float32, device=dev))
    with torch.cuda.device(dev):
        lib = _lib.load()
        nbytes = int(lib.ishara_rescore_sweep_workspace_bytes(B, N, G))
        if nbytes < 0:
            raise ValueError(f"ishara_rescore_sweep takes no B={B}, N={N}, G={G}")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        sweep_launch(lib, hyp_idx, hyp_len, B, N, Th, pointer_array(logps), M, lm_dev, eos, targets, int(targets.shape[1]), 1 if fallback else 0, grid, G,
                     best, dist, tlen, det and det["hyp_dist"], det and det["lm_score"], ws, _lib.stream())
    return (best, dist, tlen, det) if return_details else (best, dist, tlen)
