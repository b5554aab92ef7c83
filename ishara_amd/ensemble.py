"""Model ensembling for batched inference: the frame posteriors of up to 8 models fused on the device before the CTC decode.

`ishara_logits_combine` (csrc/logits_combine.hip) reads M logits buffers [B, T, C] and writes one normalised log-distribution per frame:

  z_m = logits_m / temperature_m                       lp_m = log_softmax(z_m)
  log_linear (product of experts)   s = sum_m w_m * lp_m
  linear     (mixture)              s = log sum_m w_m * exp(lp_m)        (computed max-subtracted)
  out = s - logsumexp(s)

over the models with w_m > 0; a model whose weight is not > 0 is not read, no weight > 0 gives the uniform row -log C, and with per-clip
frame counts the rows past a clip's end are not read and are written +0.  The result feeds `ctc_greedy_decode`, `ctc_beam_decode`,
`ctc_align` and `ctc_loss` of ishara_amd/ctc.py as it is: they take logits, and a normalised log-distribution is its own log-softmax up
to rounding.

  combine_reference     the formulas in fp64 numpy: the oracle of the tests
  normalise_weights     float32 [M] summing to 1
  combine_logits        device tensors in, device tensor out, on the current stream, no host synchronise
  EnsembleTFLiteModel   `BatchedTFLiteModel` for 1..8 models in one graph replay: one preprocessing, M forward passes, the fusion, then
                        that class's decode / edit distance / alignment tail

No accuracy effect on real data is measured anywhere in this repository: there is no dataset and there are no trained weights.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .tflite_batch import BatchedTFLiteModel, encode_phrase, normalized_scores
from .tflite_model import N_COLS

MAX_MODELS = 8
MODES = {"log_linear": 0, "linear": 1}


def _mode(mode) -> int:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    return MODES[mode]


def normalise_weights(weights, M: int) -> np.ndarray:
    """Ensemble weights as float32 [M] that sum to 1 (in fp64, before the cast); None: uniform.  A wrong length, a negative, NaN or Inf
    entry and an all-zero vector are refused."""
    if M < 1:
        raise ValueError(f"M={M} models")
    if weights is None:
        return np.full(M, 1.0 / M, dtype=np.float64).astype(np.float32)
    w = np.asarray(weights, dtype=np.float64)
    if w.shape != (M,):
        raise ValueError(f"weights must be {M} numbers (one per model), got shape {w.shape}")
    if not np.isfinite(w).all():
        raise ValueError(f"weights must be finite, got {w.tolist()}")
    if (w < 0).any():
        raise ValueError(f"weights must not be negative, got {w.tolist()}")
    tot = float(w.sum())
    if not tot > 0:
        raise ValueError("weights are all zero")
    return (w / tot).astype(np.float32)


def inverse_temperatures(temperatures, M: int) -> Optional[np.ndarray]:
    """The divisors tau_m > 0 as what the device multiplies by: float32 [M] of 1 / tau_m; None stays None (no multiply)."""
    if temperatures is None:
        return None
    t = np.asarray(temperatures, dtype=np.float64)
    if t.shape != (M,):
        raise ValueError(f"temperatures must be {M} numbers (one per model), got shape {t.shape}")
    if not np.isfinite(t).all() or (t <= 0).any():
        raise ValueError(f"temperatures must be finite and > 0, got {t.tolist()}")
    return (1.0 / t).astype(np.float32)


def _log_softmax64(z):
    d = z - z.max(axis=-1, keepdims=True)
    return d - np.log(np.exp(d).sum(axis=-1, keepdims=True))


def combine_reference(logits, weights=None, mode="log_linear", temperatures=None, frame_lengths=None) -> np.ndarray:
    """The fusion in fp64 numpy.  logits: M arrays [B, T, C] (or one array [M, B, T, C]); weights: M numbers taken as they are (None:
    uniform), a weight that is not > 0 leaves its model unread; temperatures: M divisors > 0, applied as the device applies them (one
    multiply by the float32 value of 1 / tau); frame_lengths: B integers, a value outside [1, T] means a clip without frames, rows past
    a clip's end are +0.  Returns float64 [B, T, C]."""
    md = _mode(mode)
    xs = [np.asarray(x) for x in logits]
    M = len(xs)
    if M < 1 or any(x.ndim != 3 or x.shape != xs[0].shape for x in xs):
        raise ValueError("logits must be M >= 1 arrays of one shape [B, T, C]")
    B, T, Cn = xs[0].shape
    w = np.full(M, 1.0 / M) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (M,):
        raise ValueError(f"weights must be {M} numbers, got shape {w.shape}")
    it = inverse_temperatures(temperatures, M)
    used = [m for m in range(M) if w[m] > 0]
    if not used:
        out = np.full((B, T, Cn), -np.log(float(Cn)))
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            lps = [_log_softmax64(xs[m].astype(np.float64) * (float(it[m]) if it is not None else 1.0)) for m in used]
            if md == 0:
                s = np.zeros((B, T, Cn))
                for m, lp in zip(used, lps):
                    s = s + w[m] * lp
            else:
                terms = np.stack([np.log(w[m]) + lp for m, lp in zip(used, lps)])
                a = terms.max(axis=0)
                s = a + np.log(np.exp(terms - a).sum(axis=0))
            out = _log_softmax64(s)
    if frame_lengths is not None:
        fl = np.asarray(frame_lengths).astype(np.int64)
        if fl.shape != (B,):
            raise ValueError(f"frame_lengths must be {B} integers, got shape {fl.shape}")
        tb = np.where((fl < 1) | (fl > T), 0, fl)
        out = np.where(np.arange(T)[None, :, None] < tb[:, None, None], out, 0.0)
    return out


def _pointer_array(tensors: Sequence[torch.Tensor]):
    """the host array of device pointers ishara_logits_combine takes"""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def combine_logits(logits, weights=None, mode="log_linear", temperatures=None, frame_lengths=None, out=None) -> torch.Tensor:
    """The fusion on the device.  logits: M <= 8 fp32 tensors [B, T, C] on one GPU (or one tensor [M, B, T, C]); weights pass through
    `normalise_weights`; temperatures are divisors tau_m > 0 (the device gets 1 / tau_m); frame_lengths as in ishara_amd/ctc.py (a host
    sequence is validated against 1..T, a device tensor is handed on unread).  Runs on the current stream without a host synchronise and
    returns `out` (allocated when None): fp32 [B, T, C], a normalised log-distribution per frame."""
    from . import ctc
    md = _mode(mode)
    xs = [ctc._logits(x) for x in logits]
    M = len(xs)
    if M < 1 or M > MAX_MODELS:
        raise ValueError(f"{M} models: the fusion takes 1..{MAX_MODELS}")
    if any(x.shape != xs[0].shape for x in xs):
        raise ValueError(f"every model's logits must have one shape, got {[tuple(x.shape) for x in xs]}")
    B, T, Cn = xs[0].shape
    if not 2 <= Cn <= ctc.MAX_CLASSES:
        raise ValueError(f"C={Cn} outside 2..{ctc.MAX_CLASSES} (one lane per class)")
    w = normalise_weights(weights, M)
    it = inverse_temperatures(temperatures, M)
    fl = None if frame_lengths is None else ctc._lengths(frame_lengths, B, T, 1, "frame_lengths", xs[0].device)
    for x in xs:
        ctc._need_gpu(x)
    dev = xs[0].device
    if any(x.device != dev for x in xs):
        raise ValueError("every model's logits must be on one device")
    xs = [x.to(torch.float32).contiguous() for x in xs]
    if out is None:
        out = torch.empty((B, T, Cn), dtype=torch.float32, device=dev)
    elif out.shape != (B, T, Cn) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous fp32 [{B}, {T}, {Cn}] tensor on {dev}")
    with torch.cuda.device(dev):
        w_d = torch.from_numpy(w).to(dev, non_blocking=True)
        it_d = None if it is None else torch.from_numpy(it).to(dev, non_blocking=True)
        _lib.check(_lib.load().ishara_logits_combine(None, _pointer_array(xs), M, B, T, Cn, _lib.ptr(w_d), _lib.ptr(it_d), md, _lib.ptr(fl),
                                                     _lib.ptr(out), _lib.stream()), "ishara_logits_combine")
    return out


class EnsembleTFLiteModel(BatchedTFLiteModel):
    """`BatchedTFLiteModel` for an ensemble: per batch ishara_preprocess_batch once, ishara_forward(training = 0) of every model into a
    logits buffer of its own, ishara_logits_combine into the buffer the decoders read, then the inherited tail (greedy or beam top-1,
    ishara_edit_distance, ishara_edit_alignment) in the same graph; staging, the two slots, the copy stream and the single host wait are
    inherited.  The models share T, C, max_label_len and the device; they may differ in dim, block counts and compute dtype.  The ensemble
    weights live on the device and are read by every replay: `set_weights` needs no new capture."""

    def __init__(self, models, weights=None, mode: str = "log_linear", temperatures=None, stats: Optional[Dict[str, tuple]] = None,
                 batch_size: int = 64, max_frames: int = 1024, use_graph: bool = True, beam_width: int = 0, lm=None, lm_alpha: float = 0.0,
                 lm_beta: float = 0.0, mbr_nbest: int = 0, mbr_temperature: float = 1.0, mbr_normalise: bool = True, rescore_nbest: int = 0,
                 rescore_lm=None, rescore_alpha: float = 0.0, rescore_beta: float = 0.0, rescore_temperature: float = 1.0):
        """rescore_*: BatchedTFLiteModel's second pass, here on the FUSED rows: the exact scores are taken under the combined logits, one
        "model" (M = 1); scoring every hypothesis under every member (rescore.rescore_models) is not wired into a wrapper."""
        models = list(models)
        M = len(models)
        if M < 1 or M > MAX_MODELS:
            raise ValueError(f"{M} models: an ensemble takes 1..{MAX_MODELS}")
        self._mode_id = _mode(mode)
        for m in models:
            if m.F != N_COLS:
                raise ValueError(f"the TFLite wrapper feeds {N_COLS} columns (92 landmarks x 3); a model has F={m.F}")
        for name, vals in (("T", [m.T for m in models]), ("C", [m.C for m in models]), ("max_label_len", [int(m._cfg.max_label_len) for m in models])):
            if len(set(vals)) != 1:
                raise ValueError(f"the models of an ensemble must share {name}, got {vals}")
        smallest = min(m.max_batch for m in models)
        if batch_size < 1 or batch_size > smallest:
            raise ValueError(f"batch_size {batch_size} outside 1..{smallest}, the smallest max_batch of the models")
        w = normalise_weights(weights, M)
        it = inverse_temperatures(temperatures, M)
        if len({m.device for m in models}) != 1:
            raise ValueError(f"the models of an ensemble must be on one device, got {[str(m.device) for m in models]}")
        super().__init__(models[0], stats=stats, batch_size=batch_size, max_frames=max_frames, use_graph=use_graph, beam_width=beam_width, lm=lm,
                         lm_alpha=lm_alpha, lm_beta=lm_beta, mbr_nbest=mbr_nbest, mbr_temperature=mbr_temperature, mbr_normalise=mbr_normalise,
                         rescore_nbest=rescore_nbest, rescore_lm=rescore_lm, rescore_alpha=rescore_alpha, rescore_beta=rescore_beta,
                         rescore_temperature=rescore_temperature)
        self.models, self.mode = models, mode
        dev = self.model.device
        self._per_model = torch.zeros((M, batch_size, self.T, self.model.C), dtype=torch.float32, device=dev)
        self._ptrs = _pointer_array([self._per_model[m] for m in range(M)])
        self._w = torch.from_numpy(w).to(dev)
        self._w_host = w
        self._inv_temp = None if it is None else torch.from_numpy(it).to(dev)

    # ---- the ensemble weights
    @property
    def weights(self) -> np.ndarray:
        return self._w_host.copy()

    def set_weights(self, weights) -> None:
        """Normalised weights written into the device array every replay reads (on the current stream; no new capture)."""
        w = normalise_weights(weights, len(self.models))
        self._w.copy_(torch.from_numpy(w))
        self._w_host = w

    # ---- device work of one batch
    def _launch_forwards(self, slot: int):
        self._launch_preprocess(slot)
        for m, mod in enumerate(self.models):
            _lib.check(mod._lib.ishara_forward(mod._h, _lib.ptr(self._x), self.batch_size, _lib.ptr(self._per_model[m]), 0, C.c_uint32(0), _lib.stream()),
                       "ishara_forward")

    def _launch_combine(self):
        _lib.check(self.model._lib.ishara_logits_combine(None, self._ptrs, len(self.models), self.batch_size, self.T, self.model.C, _lib.ptr(self._w),
                                                         _lib.ptr(self._inv_temp), self._mode_id, None, _lib.ptr(self._logits), _lib.stream()),
                   "ishara_logits_combine")

    def _launch_logits(self, slot: int):
        self._launch_forwards(slot)
        self._launch_combine()

    def _run_part(self, key, launch):
        if self.use_graph:
            self._captured(key, launch).replay()
        else:
            launch()

    # ---- public surface beyond the inherited predict_indices / __call__ / score
    def logits(self, clips) -> Dict[str, np.ndarray]:
        """What the device computed for `clips`, as numpy: x [n, T, 276] (the preprocessed input), per_model [M, n, T, C] (every model's
        logits) and combined [n, T, C] (what the decoders read).  One host wait per batch: for inspection and tests, not for throughput."""
        xs, per, comb = [], [], []
        for i, (fill, n) in enumerate(self._batches(clips)):
            s = self._stage(i, fill, n)
            self._run_part(("logits", s), lambda s=s: self._launch_logits(s))
            self._mark_consumed(s)
            xs.append(self._x[:n].cpu().numpy())
            per.append(self._per_model[:, :n].cpu().numpy())
            comb.append(self._logits[:n].cpu().numpy())
        M, T, Cn = len(self.models), self.T, self.model.C
        if not xs:
            return dict(x=np.zeros((0, T, N_COLS), np.float32), per_model=np.zeros((M, 0, T, Cn), np.float32), combined=np.zeros((0, T, Cn), np.float32))
        return dict(x=np.concatenate(xs), per_model=np.concatenate(per, axis=1), combined=np.concatenate(comb))

    def score_weights(self, clips, targets, candidates, char_to_num: Optional[Dict[str, int]] = None) -> Dict[str, np.ndarray]:
        """`score` under every weight vector of `candidates` [K, M] with the models run once: per batch the preprocessing and the M forward
        passes run once (one graph), then fusion, decode and edit distance once per candidate (a second graph, replayed K times on the
        candidate copied into the weights array on the device).  The candidates are normalised and uploaded once.  Returns mean_scores [K]
        and distances [K, n]; row k equals `set_weights(candidates[k]); score(clips, targets)`.  The object's weights are left as they were."""
        M = len(self.models)
        cand = np.stack([normalise_weights(c, M) for c in candidates]) if len(candidates) else np.zeros((0, M), np.float32)
        K = cand.shape[0]
        enc = np.stack([encode_phrase(t, char_to_num, self.L) for t in targets]) if len(targets) else np.zeros((0, self.L), np.int32)
        n_clips = (np.asarray(clips[1]).shape[0] - 1) if (isinstance(clips, tuple) and len(clips) == 2 and np.ndim(clips[1]) == 1) else len(clips)
        if enc.shape[0] != n_clips:
            raise ValueError(f"{enc.shape[0]} targets for {n_clips} clips")
        bs, T = self.batch_size, self.T
        cand_d = torch.from_numpy(cand).to(self.model.device)
        keep = self._w.clone()
        h_res = torch.empty((max(K, 1), bs * T + 3 * bs), dtype=torch.int32, pin_memory=True)
        dist = [[] for _ in range(K)]
        tlen: List[np.ndarray] = []
        for i, (fill, n) in enumerate(self._batches(clips)):
            s = self._stage(i, fill, n, enc)
            self._run_part(("forwards", s), lambda s=s: self._launch_forwards(s))
            for k in range(K):
                self._w.copy_(cand_d[k])
                self._run_part(("fuse_score", s), lambda s=s: (self._launch_combine(), self._launch_tail(s, True)))
                h_res[k].copy_(self._d_res, non_blocking=True)
            self._mark_consumed(s)
            torch.cuda.current_stream().synchronize()          # the one host wait of a batch
            r = h_res.numpy()
            for k in range(K):
                dist[k].append(r[k, bs * T + bs:bs * T + bs + n].copy())
            if K:
                tlen.append(r[0, bs * T + 2 * bs:bs * T + 2 * bs + n].copy())
        self._w.copy_(keep)
        d =np.stack([np.concatenate(x) if x else np.zeros(0, np.int32) for x in dist]).astype(np.int64) if K else np.zeros((0, n_clips), np.int64)
        tl = np.concatenate(tlen) if tlen else np.zeros(0, np.int32)
        return dict(mean_scores=np.array([normalized_scores(d[k], tl)[0] for k in range(K)], dtype=np.float64), distances=d)
