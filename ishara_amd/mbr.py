"""Minimum-Bayes-risk (MBR) decoding over the beam search's n-best list: the host reference and the device entry of `ishara_mbr_select`
(csrc/mbr_select.hip; contract in include/ishara_hip.h).

Every other decoder of this package returns the most probable hypothesis.  The quality figure of the project is the mean normalised
Levenshtein score (conv-hybrid-model.ipynb c18, `evaluation.mean_score`), and the most probable string is not the string with the smallest
expected edit distance.  MBR takes the n-best list as a sample of the posterior and returns the hypothesis whose expected distance to the
others is smallest (Goel & Byrne 2000, "Minimum Bayes-risk automatic speech recognition"):

  vote     w_j = exp((s_j - s_max) / temperature), s_max the largest finite score of the live slots; a slot whose score is not finite
           votes 0.  Or explicit weights: w_j = weights[j] where that is finite and > 0, else 0.  The votes are not normalised.
  risk     risk_i = sum_j w_j * c_ij over the live slots j in ascending order,  c_ij = d_ij (mode 0) or d_ij / max(len_j, 1) (mode 1: the
           c18 metric with the voter in the target's place), d the unit-cost Levenshtein distance
  choice   slots in ascending order, a later slot wins only with a strictly smaller risk: ties go to the lowest slot

A slot is dead (None here, hyp_len < 0 on the device) or live; dead slots are neither candidates nor voters.  A clip is not ranked and
falls back to its lowest live slot when a live hypothesis is longer than 64 symbols (status bit 0) or holds a symbol outside [0, C)
(bit 1); bit 2: no live slot at all, best = -1.

  mbr_reference          one clip in numpy: DP distances, fp64 votes (or given float32 votes and the device's float32 risk arithmetic)
  mbr_select             device tensors in, device tensors out, on the current stream, nothing waits
  pool_nbest             the n-best lists of several models (any T each) as one list: MBR across models that the frame-level fusion cannot combine
  ctc.ctc_beam_nbest_device, Model.mbr_decode, TFLiteModel / BatchedTFLiteModel / EnsembleTFLiteModel(mbr_nbest=) use them

No accuracy effect on real data is measured anywhere in this repository: there is no dataset and there are no trained weights.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_NBEST = 64             # one lane per hypothesis
MAX_HYP_LEN = 64           # MAX_PHRASE_LENGTH: one 64-bit word per hypothesis in the bit-vector edit distance
MAX_FRAMES = 4096
MAX_CLASSES = 64
STATUS_LONG, STATUS_SYMBOL, STATUS_EMPTY = 1, 2, 4
MODES = {"distance": 0, "normalised": 1}


def levenshtein_dp(a: Sequence[int], b: Sequence[int]) -> int:
    """Unit-cost Levenshtein distance by the plain two-row DP."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i] + [0] * len(b)
        for j, y in enumerate(b, 1):
            cur[j] = min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def pairwise_levenshtein(seqs: Sequence[Sequence[int]]) -> np.ndarray:
    """int64 [n, n] distances among n sequences: the same DP, row by row, for all pairs at once.  Row i of a pair's table is
    cur[j] = min(prev[j-1] + (a_i != b_j), prev[j] + 1, cur[j-1] + 1); the last term is the running minimum of (. - j) along the row."""
    n = len(seqs)
    out = np.zeros((n, n), np.int64)
    if n < 2:
        return out
    lens = np.array([len(s) for s in seqs], np.int64)
    L = max(int(lens.max()), 1)
    sym = np.full((n, L), -1, np.int64)
    for k, s in enumerate(seqs):
        sym[k, :len(s)] = s
    ii, jj = np.triu_indices(n, 1)
    a, b, la, lb = sym[ii], sym[jj], lens[ii], lens[jj]
    P, ar, rows = ii.shape[0], np.arange(L + 1), np.arange(ii.shape[0])
    prev = np.tile(ar, (P, 1))
    res = np.where(la == 0, lb, 0)
    for i in range(1, L + 1):
        best = np.minimum(prev[:, :-1] + (a[:, i - 1:i] != b), prev[:, 1:] + 1)
        v = np.concatenate([np.full((P, 1), i), best - ar[1:]], axis=1)
        prev = np.minimum.accumulate(v, axis=1) + ar
        hit = la == i
        res[hit] = prev[rows[hit], lb[hit]]
    out[ii, jj] = res
    out[jj, ii] = res
    return out


def _check_mode(mode) -> int:
    if isinstance(mode, str):
        if mode not in MODES:
            raise ValueError(f"mode must be 0, 1 or one of {sorted(MODES)}, got {mode!r}")
        return MODES[mode]
    if mode not in (0, 1):
        raise ValueError(f"mode must be 0 (edit distance) or 1 (normalised by the voter's length), got {mode!r}")
    return int(mode)


def votes_reference(live, scores=None, weights=None, inv_temp: float = 1.0) -> np.ndarray:
    """The votes in fp64 from the float32 values the device reads: exp((s - s_max) * inv_temp) or the usable explicit weights; 0 in dead slots."""
    live = np.asarray(live, dtype=bool)
    w = np.zeros(live.shape[0], np.float64)
    if weights is not None:
        v = np.asarray(weights, np.float32).astype(np.float64)
        ok = live & np.isfinite(v) & (v > 0)
        w[ok] = v[ok]
        return w
    if scores is None:
        raise ValueError("scores or weights: nothing to vote with")
    s = np.asarray(scores, np.float32).astype(np.float64)
    ok = live & np.isfinite(s)
    if ok.any():
        w[ok] = np.exp((s[ok] - s[ok].max()) * float(np.float32(inv_temp)))
    return w


def risk_float32(votes, dist, lens, live, mode: int) -> np.ndarray:
    """The device's risk arithmetic: float32, one rounding per division, multiplication and addition, voters in ascending order from +0;
    NaN in dead slots.  votes float32 [N], dist int [N, N], lens int [N]."""
    f32 = np.float32
    N = len(lens)
    risk = np.full(N, np.nan, f32)
    with np.errstate(all="ignore"):
        for i in range(N):
            if not live[i]:
                continue
            r = f32(0.0)
            for j in range(N):
                if not live[j]:
                    continue
                c = f32(dist[i][j])
                if mode == 1:
                    c = f32(c / f32(max(int(lens[j]), 1)))
                r = f32(r + f32(f32(votes[j]) * c))
            risk[i] = r
    return risk


def select(risk, live) -> int:
    """The selection rule: the first live slot, replaced only by a strictly smaller risk (a NaN never wins); -1 without a live slot."""
    best = -1
    for i in range(len(risk)):
        if live[i] and (best < 0 or risk[i] < risk[best]):
            best = i
    return best


def mbr_reference(hyps, scores=None, weights=None, inv_temp: float = 1.0, mode=0, C: int = 60, votes=None):
    """One clip on the host.  hyps: N entries, each a sequence of integers or None for a dead slot; scores / weights: N numbers (weights win);
    inv_temp = 1 / temperature; mode 0 / 1.  By default the votes and the risk are fp64.  votes=: float32 [N] votes to take as they are
    (the device's w_out): the risk is then computed in the device's float32 order and equals its bits.
    Returns (best, risk [N] with NaN in dead slots, dist int64 [N, N] with -1 in dead rows and columns, status).  A clip with status bit 0 or
    1 is not ranked: best = the lowest live slot, risk all NaN, dist all -1."""
    md = _check_mode(mode)
    N = len(hyps)
    if N < 1:
        raise ValueError("an n-best list has at least one slot")
    seqs = [None if h is None else [int(v) for v in h] for h in hyps]
    live = np.array([s is not None for s in seqs])
    lens = np.array([len(s) if s is not None else -1 for s in seqs], np.int64)
    status = 0
    if any(s is not None and len(s) > MAX_HYP_LEN for s in seqs):
        status |= STATUS_LONG
    if any(s is not None and any(v < 0 or v >= C for v in s[:MAX_HYP_LEN]) for s in seqs):
        status |= STATUS_SYMBOL
    if not live.any():
        status |= STATUS_EMPTY
    dist = np.full((N, N), -1, np.int64)
    nan = np.full(N, np.nan, np.float32 if votes is not None else np.float64)
    if status:
        return (int(np.argmax(live)) if live.any() else -1), nan, dist, status
    alive = np.nonzero(live)[0]
    dist[np.ix_(alive, alive)] = pairwise_levenshtein([seqs[i] for i in alive])
    if votes is not None:
        v = np.asarray(votes, np.float32)
        if v.shape != (N,):
            raise ValueError(f"votes must be {N} numbers, got shape {v.shape}")
        risk = risk_float32(v, dist, lens, live, md)
    else:
        if scores is None and weights is None:
            raise ValueError("scores or weights: nothing to vote with")
        w = votes_reference(live, scores, weights, inv_temp)
        cost = dist.astype(np.float64)
        if md == 1:
            cost = cost / np.maximum(lens, 1)[None, :].astype(np.float64)
        risk = nan.copy()
        for i in range(N):
            if live[i]:
                risk[i] = math.fsum(w[j] * cost[i, j] for j in range(N) if live[j])
    return select(risk, live), risk, dist, status


# ---------------------------------------------------------------------------------------------------- device side (ishara_mbr_select)
def check_device_args(N: int, T: int, C: int, mode) -> int:
    """The kernel's limits (include/ishara_hip.h), checked before any launch or capture; returns the mode as 0 / 1."""
    md = _check_mode(mode)
    if not 1 <= N <= MAX_NBEST:
        raise ValueError(f"N={N} hypotheses per clip outside 1..{MAX_NBEST} (one lane per hypothesis)")
    if not 1 <= T <= MAX_FRAMES:
        raise ValueError(f"T={T} outside 1..{MAX_FRAMES}")
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"C={C} outside 2..{MAX_CLASSES}")
    return md


def inverse_temperature(temperature) -> float:
    """1 / temperature as the float32 the device multiplies by; a temperature that is not finite and > 0 is refused."""
    t = float(temperature)
    if not math.isfinite(t) or t <= 0:
        raise ValueError(f"temperature must be finite and > 0, got {temperature!r}")
    return float(np.float32(1.0 / t))


def _cuda(t, dtype, shape, what: str):
    import torch
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a torch tensor on the GPU, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{what} must be on the GPU (the selection kernel has no CPU path; mbr.mbr_reference is the host reference)")
    if t.dtype != dtype:
        raise ValueError(f"{what} must be {dtype}, got {t.dtype}")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be {list(shape)}, got {list(t.shape)}")
    return t.contiguous()


def launch(lib, hyp_idx, hyp_len, hyp_score, weights, inv_temp, B: int, N: int, T: int, C: int, mode: int, out_idx, out_len, best, risk, w_out,
           dist, status, stream) -> None:
    """One ishara_mbr_select launch on `stream` (graph-capturable)."""
    from . import _lib
    _lib.check(lib.ishara_mbr_select(_lib.ptr(hyp_idx), _lib.ptr(hyp_len), _lib.ptr(hyp_score), _lib.ptr(weights), _lib.ptr(inv_temp), B, N, T, C, mode,
                                     _lib.ptr(out_idx), _lib.ptr(out_len), _lib.ptr(best), _lib.ptr(risk), _lib.ptr(w_out), _lib.ptr(dist),
                                     _lib.ptr(status), stream), "ishara_mbr_select")


def mbr_select(hyp_idx, hyp_len, hyp_score=None, weights=None, inv_temp=None, mode=0, C: int = 60, return_details: bool = False):
    """The selection on the device.  hyp_idx int32 [B, N, T], hyp_len int32 [B, N] and hyp_score fp32 [B, N] as ishara_ctc_beam_decode writes
    them (ctc.ctc_beam_nbest_device, pool_nbest); weights fp32 [B, N]: explicit votes in place of the scores; inv_temp: None (1.0), a number,
    or a one-element fp32 device tensor that is handed on unread; mode 0 / 1 (or "distance" / "normalised"); C: the class count the symbols
    are checked against.  Runs on the current stream, nothing waits.
    Returns (out_idx int32 [B, T], out_len int32 [B], best int32 [B]): the greedy layout ishara_edit_distance / ishara_edit_alignment read;
    with return_details also a dict of risk fp32 [B, N], votes fp32 [B, N], dist int32 [B, N, N] and status int32 [B]."""
    import torch
    from . import _lib
    hyp_idx = _cuda(hyp_idx, torch.int32, None, "hyp_idx")
    if hyp_idx.ndim != 3:
        raise ValueError(f"hyp_idx must be [B, N, T], got {tuple(hyp_idx.shape)}")
    B, N, T = hyp_idx.shape
    md = check_device_args(N, T, C, mode)
    dev = hyp_idx.device
    hyp_len = _cuda(hyp_len, torch.int32, (B, N), "hyp_len")
    if hyp_score is None and weights is None:
        raise ValueError("hyp_score or weights: nothing to vote with")
    hyp_score = None if hyp_score is None else _cuda(hyp_score, torch.float32, (B, N), "hyp_score")
    weights = None if weights is None else _cuda(weights, torch.float32, (B, N), "weights")
    if inv_temp is not None and not isinstance(inv_temp, torch.Tensor):
        v = float(inv_temp)
        if not math.isfinite(v) or v <= 0:
            raise ValueError(f"inv_temp must be finite and > 0, got {inv_temp!r}")
        inv_temp = torch.full((1,), v, dtype=torch.float32, device=dev)
    elif inv_temp is not None:
        inv_temp = _cuda(inv_temp, torch.float32, (1,), "inv_temp")
    for t, what in ((hyp_len, "hyp_len"), (hyp_score, "hyp_score"), (weights, "weights"), (inv_temp, "inv_temp")):
        if t is not None and t.device != dev:
            raise ValueError(f"hyp_idx and {what} must be on one device")
    out_idx = torch.empty((B, T), dtype=torch.int32, device=dev)
    out_len = torch.empty(B, dtype=torch.int32, device=dev)
    best = torch.empty(B, dtype=torch.int32, device=dev)
    det = None
    if return_details:
        det = dict(risk=torch.empty((B, N), dtype=torch.float32, device=dev), votes=torch.empty((B, N), dtype=torch.float32, device=dev),
                   dist=torch.empty((B, N, N), dtype=torch.int32, device=dev), status=torch.empty(B, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        launch(_lib.load(), hyp_idx, hyp_len, hyp_score, weights, inv_temp, B, N, T, C, md, out_idx, out_len, best,
               det and det["risk"], det and det["votes"], det and det["dist"], det and det["status"], _lib.stream())
    return (out_idx, out_len, best, det) if return_details else (out_idx, out_len, best)


def pool_nbest(lists, model_weights=None):
    """The n-best lists of several models as one: `lists` is a sequence of (hyp_idx [B, N_m, T_m] int32, hyp_len [B, N_m] int32, hyp_score
    [B, N_m] fp32) on one device (CPU tensors work too), concatenated along the slot axis in the order given.  The models may differ in T:
    rows are padded with -1 to the longest.  model_weights: one number > 0 per model; a_m enters as + log a_m on that model's scores (a
    dead slot keeps -inf).  More than 64 slots in all are refused.  The pooled list is ranked within each model only: MBR's tie rule then
    prefers the earlier model."""
    import torch
    lists = list(lists)
    if not lists:
        raise ValueError("no n-best lists to pool")
    if model_weights is not None:
        a = np.asarray(model_weights, np.float64)
        if a.shape != (len(lists),):
            raise ValueError(f"model_weights must be {len(lists)} numbers (one per list), got shape {a.shape}")
        if not np.isfinite(a).all() or (a <= 0).any():
            raise ValueError(f"model_weights must be finite and > 0, got {a.tolist()}")
    idxs, lens, scs = [], [], []
    B, dev = None, None
    for m, item in enumerate(lists):
        if len(item) != 3:
            raise ValueError(f"list {m}: expected (hyp_idx, hyp_len, hyp_score)")
        ix, ln, sc = (torch.as_tensor(t) for t in item)
        if ix.ndim != 3 or ix.dtype != torch.int32:
            raise ValueError(f"list {m}: hyp_idx must be int32 [B, N, T], got {tuple(ix.shape)} {ix.dtype}")
        if tuple(ln.shape) != tuple(ix.shape[:2]) or ln.dtype != torch.int32:
            raise ValueError(f"list {m}: hyp_len must be int32 {list(ix.shape[:2])}, got {tuple(ln.shape)} {ln.dtype}")
        if tuple(sc.shape) != tuple(ix.shape[:2]) or sc.dtype != torch.float32:
            raise ValueError(f"list {m}: hyp_score must be fp32 {list(ix.shape[:2])}, got {tuple(sc.shape)} {sc.dtype}")
        if B is None:
            B, dev = ix.shape[0], ix.device
        if ix.shape[0] != B:
            raise ValueError(f"list {m} has {ix.shape[0]} clips, list 0 has {B}")
        if ix.device != dev or ln.device != dev or sc.device != dev:
            raise ValueError("every n-best list must be on one device")
        if model_weights is not None:
            sc = sc + float(np.float32(math.log(a[m])))
        idxs.append(ix); lens.append(ln); scs.append(sc)
    total = sum(ix.shape[1] for ix in idxs)
    if total > MAX_NBEST:
        raise ValueError(f"{total} pooled hypotheses per clip: the selection takes at most {MAX_NBEST}")
    T = max(ix.shape[2] for ix in idxs)
    idxs = [ix if ix.shape[2] == T else torch.nn.functional.pad(ix, (0, T - ix.shape[2]), value=-1) for ix in idxs]
    return torch.cat(idxs, dim=1).contiguous(), torch.cat(lens, dim=1).contiguous(), torch.cat(scs, dim=1).contiguous()


def nbest_to_lists(hyp_idx, hyp_len) -> List[List[Optional[List[int]]]]:
    """Host arrays [B, N, T] / [B, N] as what mbr_reference takes: per clip N entries, None for a dead slot, lengths clamped to T."""
    ix, ln = np.asarray(hyp_idx), np.asarray(hyp_len)
    T = ix.shape[2]
    return [[None if ln[b, n] < 0 else ix[b, n, :min(int(ln[b, n]), T)].tolist() for n in range(ix.shape[1])] for b in range(ix.shape[0])]
