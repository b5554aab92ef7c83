"""Batched counterpart of `TFLiteModel`: many ragged raw clips per call, and the test-set score of conv-hybrid-model.ipynb c18:1-15
computed on the device.

`TFLiteModel` runs the reference's `serving_default` signature one clip at a time (B = 1).  The reference's accuracy figure comes from a
loop over the test set (c18) that calls it per clip, maps the one-hot output back to characters and averages
(len(target) - Levenshtein(pred, target)) / len(target) on the host.  `BatchedTFLiteModel` runs `batch_size` clips per hipGraph replay:

  packed raw clips [N, 276] + offsets [B+1] --ishara_preprocess_batch--> x [B, T, 276] --ishara_forward(training=0)--> logits
  --ishara_greedy_decode (ishara_ctc_beam_decode top-1 with beam_width > 0)--> indices, lengths [--ishara_edit_distance (len < 3 fallback, pad-59 targets)--> dist, tlen]

Per batch the host packs the clips into one pinned staging buffer (offsets | targets | raw frames), copies it with one non-blocking
H2D copy on a copy stream, replays the graph on the current stream and copies the results (indices | lengths | dist | tlen) back with one
D2H copy.  Two staging slots: batch i+1 is packed and copied while batch i replays; the host waits once per batch.  A last partial batch
fills its unused slots with empty clips (equal offsets), whose outputs are dropped.  Each clip's result equals `TFLiteModel(...)(clip)`:
the preprocessing is bit-identical per clip, and an inference-mode forward pass has no cross-sample statistics.

`score(breakdown=True)` appends ishara_edit_alignment (fallback = 1) to the captured sequence: per-clip operation counts and per-position
records in a result buffer of their own (ops | aligned | inserted, a second D2H copy in front of the same host wait), and one 60 x 60
confusion matrix that stays on the device for the whole test set (zeroed before the first batch, read once after the last).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import stream as _stream
from .evaluation import ErrorReport
from .model import Model
from .tflite_model import FALLBACK_PHRASE, N_COLS, PARTS, _beam_launch, _beam_setup, _mbr_launch, _mbr_setup, _set_mbr_temperature, refuse_frame_lengths
from .tflite_model import _rescore_launch, _rescore_search, _rescore_setup, _set_rescore

PAD_TOKEN_IDX = 59           # c1:5: the targets' padding; never a decoded index (the blank is C - 1 = 59)
MAX_SCORE_LABEL_LEN = 64     # one wavefront lane per target symbol (ishara_edit_distance)
_ROW_BYTES = N_COLS * 4


def _align(n: int, a: int) -> int:
    return (n + a - 1) // a * a


# ---------------------------------------------------------------------------------------------------- host helpers (no device)
def check_clip(x, max_frames: int) -> np.ndarray:
    """One raw clip as float32 [n, 276], n <= max_frames (the checks of TFLiteModel.predict_indices)."""
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] != N_COLS:
        raise ValueError(f"inputs must be [n_frames, {N_COLS}], got {x.shape}")
    if x.shape[0] > max_frames:
        raise ValueError(f"clip of {x.shape[0]} frames exceeds max_frames={max_frames}")
    return x


def batch_offsets(lengths: Sequence[int], batch_size: int) -> np.ndarray:
    """int64 [batch_size + 1] row offsets of clips packed back to back; slots past len(lengths) are empty clips (equal offsets)."""
    if len(lengths) > batch_size:
        raise ValueError(f"{len(lengths)} clips in a batch of {batch_size}")
    off = np.zeros(batch_size + 1, dtype=np.int64)
    off[1:len(lengths) + 1] = np.cumsum(np.asarray(lengths, dtype=np.int64))
    off[len(lengths) + 1:] = off[len(lengths)]
    return off


def pack_clips(clips: Sequence[np.ndarray], raw: np.ndarray, offsets: np.ndarray) -> int:
    """Copy checked clips back to back into raw [capacity, 276]; fill offsets [batch_size + 1] (padding slots empty).  Returns the rows used."""
    off = batch_offsets([c.shape[0] for c in clips], offsets.shape[0] - 1)
    rows = int(off[-1])
    if rows > raw.shape[0]:
        raise ValueError(f"{rows} frames exceed the staging capacity of {raw.shape[0]}")
    for c, o in zip(clips, off[:-1]):
        raw[o:o + c.shape[0]] = c
    offsets[:] = off
    return rows


def check_packed(frames, offsets, max_frames: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pre-packed input (frames [N, 276] float32, offsets [B + 1] int64, non-decreasing, inside [0, N], clips of at most max_frames)."""
    frames = np.asarray(frames, dtype=np.float32)
    offsets = np.asarray(offsets)
    if frames.ndim != 2 or frames.shape[1] != N_COLS:
        raise ValueError(f"packed frames must be [N, {N_COLS}], got {frames.shape}")
    if offsets.ndim != 1 or offsets.shape[0] < 1 or not np.issubdtype(offsets.dtype, np.integer):
        raise ValueError("offsets must be a 1-D integer array [B + 1]")
    offsets = offsets.astype(np.int64)
    n = np.diff(offsets)
    if offsets[0] < 0 or offsets[-1] > frames.shape[0] or (n < 0).any():
        raise ValueError(f"offsets must be non-decreasing inside [0, {frames.shape[0]}]")
    if n.size and n.max() > max_frames:
        raise ValueError(f"clip of {int(n.max())} frames exceeds max_frames={max_frames}")
    return frames, offsets


def encode_phrase(target, char_to_num: Optional[Dict[str, int]], max_len: int) -> np.ndarray:
    """A target phrase as int32 [max_len] padded with 59: a string through char_to_num (c1:3-9), or an index sequence."""
    if isinstance(target, str):
        if char_to_num is None:
            raise ValueError("string targets need char_to_num")
        unknown = sorted({ch for ch in target if ch not in char_to_num})
        if unknown:
            raise ValueError(f"target {target!r}: characters {unknown} are not in char_to_num")
        idx = np.array([char_to_num[ch] for ch in target], dtype=np.int64)
    else:
        idx = np.asarray(target)
        if idx.ndim != 1 or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
            raise ValueError("an index target must be a 1-D integer sequence")
        idx = idx.astype(np.int64)
    if idx.size == 0:
        raise ValueError("empty target: the score divides by its length (c18:9)")
    if idx.size > max_len:
        raise ValueError(f"target of {idx.size} symbols exceeds max_label_len={max_len}")
    if (idx < 0).any() or (idx >= PAD_TOKEN_IDX).any():
        raise ValueError(f"target indices must lie in [0, {PAD_TOKEN_IDX})")
    out = np.full(max_len, PAD_TOKEN_IDX, dtype=np.int32)
    out[:idx.size] = idx
    return out


def apply_fallback(idx: np.ndarray) -> np.ndarray:
    """The wrapper's rule (c13:22-23): a decode shorter than 3 symbols becomes the constant phrase."""
    return FALLBACK_PHRASE if idx.shape[0] < 3 else idx


def one_hot(idx: np.ndarray) -> np.ndarray:
    """tf.one_hot(x, 59) (c13:24): index 59 -> zero row."""
    out = np.zeros((idx.shape[0], 59), dtype=np.float32)
    ok = idx < 59
    out[np.arange(idx.shape[0])[ok], idx[ok]] = 1.0
    return out


def normalized_scores(dist: np.ndarray, tlen: np.ndarray) -> Tuple[float, np.ndarray]:
    """(len(target) - distance) / len(target) per clip and np.sum(scores) / len(scores) (c18:9-15), in float64 as the host scorer does."""
    scores = [(int(t) - int(d)) / int(t) for d, t in zip(dist, tlen)]
    mean = float(np.sum(scores) / len(scores)) if scores else 0.0
    return mean, np.asarray(scores, dtype=np.float64)


# ---------------------------------------------------------------------------------------------------- device runner
class BatchedTFLiteModel:
    def __init__(self, model: Model, stats: Optional[Dict[str, tuple]] = None, batch_size: int = 64, max_frames: int = 1024,
                 use_graph: bool = True, beam_width: int = 0, lm=None, lm_alpha: float = 0.0, lm_beta: float = 0.0, mbr_nbest: int = 0,
                 mbr_temperature: float = 1.0, mbr_normalise: bool = True, rescore_nbest: int = 0, rescore_lm=None, rescore_alpha: float = 0.0,
                 rescore_beta: float = 0.0, rescore_temperature: float = 1.0):
        """beam_width / lm / lm_alpha / lm_beta as for TFLiteModel: 0 keeps the greedy decode; > 0 captures the beam decoder (top-1) in
        its place, and predict_indices / __call__ / score() work on the beam's top-1.  mbr_nbest / mbr_temperature / mbr_normalise as for
        TFLiteModel: with mbr_nbest >= 2 the beam search keeps that many hypotheses, ishara_mbr_select follows it in the graph and writes
        the indices and lengths the tail reads, so everything downstream works on the minimum-Bayes-risk choice.  rescore_nbest /
        rescore_lm / rescore_alpha / rescore_beta / rescore_temperature as for TFLiteModel: with rescore_nbest >= 2 the exact scores and
        ishara_nbest_rescore_p follow the beam search in the graph, and predict_indices / __call__ / score() / score(breakdown=True) work
        on the rescored choice; set_rescore rewrites the parameters on the device and score_rescore_grid sweeps them in one launch."""
        if model.F != N_COLS:
            raise ValueError(f"the TFLite wrapper feeds {N_COLS} columns (92 landmarks x 3); model has F={model.F}")
        if batch_size < 1 or batch_size > model.max_batch:
            raise ValueError(f"batch_size {batch_size} outside 1..max_batch={model.max_batch}")
        if max_frames < 1 or max_frames > 8192:
            raise ValueError(f"max_frames {max_frames} outside 1..8192")
        L = int(model._cfg.max_label_len)
        if L < 1 or L > MAX_SCORE_LABEL_LEN:
            raise ValueError(f"max_label_len {L} outside 1..{MAX_SCORE_LABEL_LEN} (device scoring: one wavefront lane per target symbol)")
        if model.device is None:
            raise ValueError("the model has no device: build it with device='cuda:N'")
        self.model, self.batch_size, self.max_frames, self.T, self.L = model, batch_size, max_frames, model.T, L
        dev, bs, T = model.device, batch_size, model.T
        mean = np.concatenate([(stats[n][0] if stats else np.zeros((c, 3), np.float32)).reshape(-1) for n, c in PARTS])
        std = np.concatenate([(stats[n][1] if stats else np.ones((c, 3), np.float32)).reshape(-1) for n, c in PARTS])
        self._mean = torch.from_numpy(mean.astype(np.float32)).to(dev)
        self._std = torch.from_numpy(std.astype(np.float32)).to(dev)
        # staging layout (bytes), the same on the host (pinned) and on the device: offsets int64 [bs+1] | targets int32 [bs, L] | raw f32 [cap, 276]
        self._cap = bs * max_frames
        self._tgt_at = _align((bs + 1) * 8, 256)
        self._raw_at = _align(self._tgt_at + bs * L * 4, 256)
        nbytes = self._raw_at + self._cap * _ROW_BYTES
        self._h_in = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        self._d_in = [torch.zeros(nbytes, dtype=torch.uint8, device=dev) for _ in range(2)]
        for d in self._d_in:                     # every slot starts as bs empty clips with all-pad targets
            self._off(d).zero_()
            self._tgt(d).fill_(PAD_TOKEN_IDX)
        # results: indices int32 [bs, T] | lengths [bs] | dist [bs] | tlen [bs], one D2H copy per batch
        self._d_res = torch.zeros(bs * T + 3 * bs, dtype=torch.int32, device=dev)
        self._h_res = [torch.empty(bs * T + 3 * bs, dtype=torch.int32, pin_memory=True) for _ in range(2)]
        self._idx = self._d_res[:bs * T].view(bs, T)
        self._len, self._dist, self._tlen = (self._d_res[bs * T + k * bs: bs * T + (k + 1) * bs] for k in range(3))
        self._x = torch.zeros((bs, T, N_COLS), dtype=torch.float32, device=dev)
        self._logits = torch.zeros((bs, T, model.C), dtype=torch.float32, device=dev)
        self._beam = _beam_setup(model, bs, beam_width, lm, lm_alpha, lm_beta)
        self._mbr = _mbr_setup(model, bs, self._beam, mbr_nbest, mbr_temperature, mbr_normalise)
        self._rescore = _rescore_setup(model, bs, self._beam, self._mbr, rescore_nbest, rescore_lm, rescore_alpha, rescore_beta, rescore_temperature)
        self._sweep = {}                         # score_rescore_grid's buffers by grid size, made on first use
        self._copy_stream = torch.cuda.Stream(device=dev)
        self._copied = [torch.cuda.Event() for _ in range(2)]
        self._consumed = [None, None]            # event after the replay that last read a device slot
        self._done = [torch.cuda.Event() for _ in range(2)]
        self.use_graph = use_graph
        self._graphs: Dict[Tuple[int, bool, bool], torch.cuda.CUDAGraph] = {}
        self._brk = None                         # score(breakdown=True)'s buffers, made on first use

    def _breakdown_buffers(self):
        """ops int32 [bs, 4] | aligned [bs, L] | inserted [bs, L + 1] with two pinned copies, the confusion matrix and the kernel's workspace."""
        if self._brk is None:
            bs, L, dev = self.batch_size, self.L, self.model.device
            n = bs * (4 + L + L + 1)
            d = torch.zeros(n, dtype=torch.int32, device=dev)
            need = int(self.model._lib.ishara_edit_alignment_workspace_bytes(bs, self.T))
            if need < 0:
                raise ValueError(f"edit alignment: batch_size={bs} T={self.T} unsupported")
            ws_owner, ws = _lib.aligned(need, dev)
            self._brk = dict(d=d, h=[torch.empty(n, dtype=torch.int32, pin_memory=True) for _ in range(2)],
                             ops=d[:bs * 4].view(bs, 4), aligned=d[bs * 4:bs * (4 + L)].view(bs, L), inserted=d[bs * (4 + L):].view(bs, L + 1),
                             conf=torch.zeros((60, 60), dtype=torch.int32, device=dev), ws_owner=ws_owner, ws=ws)
        return self._brk

    # ---- views of a staging buffer (host or device)
    def _off(self, buf):
        return buf[:(self.batch_size + 1) * 8].view(torch.int64)

    def _tgt(self, buf):
        return buf[self._tgt_at:self._tgt_at + self.batch_size * self.L * 4].view(torch.int32).view(self.batch_size, self.L)

    def _raw(self, buf):
        return buf[self._raw_at:].view(torch.float32).view(self._cap, N_COLS)

    # ---- device work of one batch
    def _launch(self, slot: int, scoring: bool, breakdown: bool = False):
        self._launch_logits(slot)
        self._launch_tail(slot, scoring, breakdown)

    def _launch_preprocess(self, slot: int):
        d = self._d_in[slot]
        _lib.check(self.model._lib.ishara_preprocess_batch(_lib.ptr(self._raw(d)), self._cap, _lib.ptr(self._off(d)), self.batch_size, self.max_frames,
                                                           _lib.ptr(self._mean), _lib.ptr(self._std), _lib.ptr(self._x), self.T, _stream()),
                   "ishara_preprocess_batch")

    def _launch_logits(self, slot: int):
        """device slot `slot` -> self._logits, the buffer the decoders read (EnsembleTFLiteModel: every model's forward pass and the fusion)"""
        self._launch_preprocess(slot)
        _lib.check(self.model._lib.ishara_forward(self.model._h, _lib.ptr(self._x), self.batch_size, _lib.ptr(self._logits), 0, C.c_uint32(0), _stream()),
                   "ishara_forward")

    def _launch_tail(self, slot: int, scoring: bool, breakdown: bool = False):
        lib, m, d, bs = self.model._lib, self.model, self._d_in[slot], self.batch_size
        st = _stream()
        if self._beam is None:
            _lib.check(lib.ishara_greedy_decode(_lib.ptr(self._logits), bs, self.T, m.C, m.C - 1, _lib.ptr(self._idx), _lib.ptr(self._len), st),
                       "ishara_greedy_decode")
        elif self._rescore is not None:
            _rescore_launch(m, self._beam, self._rescore, self._mbr, self._logits, bs, self._idx, self._len, st)
        elif self._mbr is not None:
            _mbr_launch(m, self._beam, self._mbr, self._logits, bs, self._idx, self._len, st)
        else:
            _beam_launch(m, self._beam, self._logits, bs, self._idx, self._len, st)
        if scoring:
            _lib.check(lib.ishara_edit_distance(_lib.ptr(self._idx), _lib.ptr(self._len), bs, self.T, _lib.ptr(self._tgt(d)), self.L,
                                                _lib.ptr(self._dist), _lib.ptr(self._tlen), st), "ishara_edit_distance")
        if breakdown:
            self._launch_alignment(slot, bs)

    def _launch_alignment(self, slot: int, n: int):
        """ishara_edit_alignment (fallback = 1) of the first n clips of the batch in device slot `slot`, adding to the object's matrix."""
        k = self._breakdown_buffers()
        _lib.check(self.model._lib.ishara_edit_alignment(_lib.ptr(self._idx), _lib.ptr(self._len), n, self.T, _lib.ptr(self._tgt(self._d_in[slot])),
                                                         self.L, 1, _lib.ptr(k["ops"]), _lib.ptr(k["aligned"]), _lib.ptr(k["inserted"]),
                                                         _lib.ptr(k["conf"]), k["ws"], _stream()), "ishara_edit_alignment")

    def _graph(self, slot: int, scoring: bool, breakdown: bool = False):
        return self._captured((slot, scoring, breakdown), lambda: self._launch(slot, scoring, breakdown), breakdown)

    def _captured(self, key, launch, breakdown: bool = False):
        """The graph of `launch()` under `key`, captured on first use."""
        if key not in self._graphs:              # as TFLiteModel._capture: warm-up outside the capture, then capture once
            conf = self._breakdown_buffers()["conf"].clone() if breakdown else None      # the warm-up launch adds to the matrix: put it back
            side = torch.cuda.Stream(device=self.model.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                launch()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launch()
            if breakdown:
                self._brk["conf"].copy_(conf)
            self._graphs[key] = g
        return self._graphs[key]

    def _run(self, slot: int, scoring: bool, breakdown: bool = False, n: Optional[int] = None):
        """The device sequence on the current stream, on the inputs already in device slot `slot`.  With breakdown, n < batch_size clips (the
        last, partial batch): the empty padding slots must not reach the confusion matrix, so the alignment is launched for n clips behind
        the sequence without it."""
        whole = breakdown and (n is None or n == self.batch_size)
        if self.use_graph:
            self._graph(slot, scoring, whole).replay()
        else:
            self._launch(slot, scoring, whole)
        if breakdown and not whole:
            self._launch_alignment(slot, n)

    # ---- host pipeline
    def _batches(self, clips):
        """Yield (fill(raw, offsets) -> rows, clip count) per batch for a list of clips or pre-packed (frames, offsets)."""
        bs = self.batch_size
        if isinstance(clips, tuple) and len(clips) == 2 and np.ndim(clips[1]) == 1:
            frames, offsets = check_packed(clips[0], clips[1], self.max_frames)
            n = offsets.shape[0] - 1
            for b0 in range(0, n, bs):
                off = offsets[b0:min(b0 + bs, n) + 1]

                def fill(raw, out_off, off=off):
                    rows = int(off[-1] - off[0])
                    if rows:
                        raw[:rows] = frames[off[0]:off[-1]]
                    out_off[:off.shape[0]] = off - off[0]
                    out_off[off.shape[0]:] = rows
                    return rows
                yield fill, off.shape[0] - 1
        else:
            clips = [check_clip(c, self.max_frames) for c in clips]
            for b0 in range(0, len(clips), bs):
                part = clips[b0:b0 + bs]
                yield (lambda raw, out_off, part=part: pack_clips(part, raw, out_off)), len(part)

    def _stage(self, i: int, fill, n: int, targets=None) -> int:
        """Pack batch i (n clips, with its rows of `targets` when scoring) into its pinned slot and copy it to the device slot on the copy
        stream; the current stream waits for the copy.  Returns the slot."""
        s, bs = i & 1, self.batch_size
        h, d = self._h_in[s], self._d_in[s]
        # the pinned slot is free: the batch that used it two steps ago was collected (its `done` waited on its copy)
        rows = fill(self._raw(h).numpy(), self._off(h).numpy())
        if targets is not None:
            t = self._tgt(h).numpy()
            t[:n] = targets[i * bs:i * bs + n]
            t[n:] = PAD_TOKEN_IDX
        nbytes = self._raw_at + rows * _ROW_BYTES
        with torch.cuda.stream(self._copy_stream):
            if self._consumed[s] is not None:    # the replay that last read this device slot
                self._copy_stream.wait_event(self._consumed[s])
            d[:nbytes].copy_(h[:nbytes], non_blocking=True)
            self._copied[s].record(self._copy_stream)
        torch.cuda.current_stream().wait_event(self._copied[s])
        return s

    def _mark_consumed(self, s: int):
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        self._consumed[s] = ev

    def _process(self, clips, targets=None, breakdown: bool = False):
        """Run every batch; returns the host results per batch: (indices [n, T], lengths, dist, tlen), with breakdown followed by
        (ops [n, 4], aligned [n, L], inserted [n, L + 1])."""
        scoring = targets is not None
        cur = torch.cuda.current_stream()
        out, pending = [], None
        for i, (fill, n) in enumerate(self._batches(clips)):
            s = self._stage(i, fill, n, targets)
            self._run(s, scoring, breakdown, n)
            self._mark_consumed(s)
            self._h_res[s].copy_(self._d_res, non_blocking=True)
            if breakdown:
                self._brk["h"][s].copy_(self._brk["d"], non_blocking=True)
            self._done[s].record(cur)
            if pending is not None:
                out.append(self._collect(*pending))
            pending = (s, n, breakdown)
        if pending is not None:
            out.append(self._collect(*pending))
        return out

    def _collect(self, s: int, n: int, breakdown: bool = False):
        self._done[s].synchronize()                  # the one host wait of a batch
        r = self._h_res[s].numpy()
        bs, T = self.batch_size, self.T
        idx = r[:bs * T].reshape(bs, T)[:n].copy()
        ln, dist, tlen = (r[bs * T + k * bs: bs * T + k * bs + n].copy() for k in range(3))
        if breakdown:
            k, L = self._brk["h"][s].numpy(), self.L
            return (idx, ln, dist, tlen, k[:bs * 4].reshape(bs, 4)[:n].copy(), k[bs * 4:bs * (4 + L)].reshape(bs, L)[:n].copy(),
                    k[bs * (4 + L):].reshape(bs, L + 1)[:n].copy())
        return idx, ln, dist, tlen

    # ---- public surface
    def set_mbr_temperature(self, temperature: float) -> None:
        """1 / temperature written into the device float every replay reads (on the current stream; no new capture)."""
        _set_mbr_temperature(self._mbr, temperature)

    def set_rescore(self, weight=None, alpha=None, beta=None, temperature=None) -> None:
        """The second pass's parameters (the weight on the exact score, alpha, beta, the posterior's temperature; None: as it is) written
        into the device floats every replay reads (on the current stream; no new capture)."""
        _set_rescore(self._rescore, weight, alpha, beta, temperature)

    def _sweep_buffers(self, G: int):
        """grid fp32 [G, 3] on the device and best [G, bs] | dist [G, bs] | tlen [bs] as one int32 result buffer with its pinned copy"""
        if G not in self._sweep:
            bs, dev = self.batch_size, self.model.device
            d = torch.zeros(2 * G * bs + bs, dtype=torch.int32, device=dev)
            need = int(self.model._lib.ishara_rescore_sweep_workspace_bytes(bs, self._rescore.nbest, G))
            if need < 0:
                raise ValueError(f"ishara_rescore_sweep takes no batch_size={bs}, N={self._rescore.nbest}, G={G}")
            ws_owner, ws = _lib.aligned(need, dev) if need else (None, None)
            self._sweep[G] = dict(grid=torch.zeros((G, 3), dtype=torch.float32, device=dev), d=d, h=torch.empty(2 * G * bs + bs, dtype=torch.int32, pin_memory=True),
                                  best=d[:G * bs].view(G, bs), dist=d[G * bs:2 * G * bs].view(G, bs), tlen=d[2 * G * bs:], ws_owner=ws_owner, ws=ws)
        return self._sweep[G]

    def _launch_sweep(self, slot: int, G: int):
        """device slot `slot` -> logits -> the n-best and its exact scores -> one ishara_rescore_sweep over the object's grid buffer"""
        from . import rescore
        k, cfg, m, bs = self._sweep_buffers(G), self._rescore, self.model, self.batch_size
        self._launch_logits(slot)
        _rescore_search(m, self._beam, cfg, self._logits, bs, _stream())
        _lib.check(m._lib.ishara_rescore_sweep(_lib.ptr(cfg.hyp_idx), _lib.ptr(cfg.hyp_len), bs, cfg.nbest, self.T, cfg.ptrs, 1,
                                               _lib.ptr(cfg.lm.logp) if cfg.lm is not None else None, _lib.ptr(cfg.lm.next) if cfg.lm is not None else None,
                                               cfg.lm.S if cfg.lm is not None else 0, cfg.lm.start if cfg.lm is not None else 0, m.C if cfg.lm is not None else 0,
                                               cfg.eos, _lib.ptr(self._tgt(self._d_in[slot])), self.L, 1, _lib.ptr(k["grid"]), G, _lib.ptr(k["best"]),
                                               _lib.ptr(k["dist"]), _lib.ptr(k["tlen"]), None, None, k["ws"], _stream()), "ishara_rescore_sweep")

    def score_rescore_grid(self, clips, targets, grid, char_to_num: Optional[Dict[str, int]] = None) -> Dict[str, np.ndarray]:
        """`score` under every row (weight, alpha, beta) of `grid` [G, 3] (rescore.sweep_grid([weights], alphas, betas)) with everything
        run once: per batch ONE graph of preprocessing, forward, beam search, exact scores and one ishara_rescore_sweep, then one D2H copy.
        Returns mean_scores [G], distances [G, n] and best [G, n] (the slot of the beam's n-best that tops the rescored list).  Row g equals
        `set_rescore(*grid[g]); score(clips, targets)`; the object's own parameters are left as they were (they are not touched).  The
        sweep covers the top-1 choice only: with mbr_nbest set, score() reports the minimum-Bayes-risk vote, which this does not follow."""
        if self._rescore is None:
            raise ValueError("score_rescore_grid: the wrapper was built without rescore_nbest")
        grid = np.ascontiguousarray(grid, dtype=np.float32)
        if grid.ndim != 2 or grid.shape[1] != 3 or not 1 <= grid.shape[0] <= 65536:
            raise ValueError(f"grid must be [G, 3] rows of (weight, alpha, beta) with 1 <= G <= 65536, got {grid.shape}")
        G = grid.shape[0]
        enc = np.stack([encode_phrase(t, char_to_num, self.L) for t in targets]) if len(targets) else np.zeros((0, self.L), np.int32)
        n_clips = (np.asarray(clips[1]).shape[0] - 1) if (isinstance(clips, tuple) and len(clips) == 2 and np.ndim(clips[1]) == 1) else len(clips)
        if enc.shape[0] != n_clips:
            raise ValueError(f"{enc.shape[0]} targets for {n_clips} clips")
        k, bs = self._sweep_buffers(G), self.batch_size
        k["grid"].copy_(torch.from_numpy(grid))
        best, dist, tlen = [], [], []
        for i, (fill, n) in enumerate(self._batches(clips)):
            s = self._stage(i, fill, n, enc)
            if self.use_graph:
                self._captured(("sweep", s, G), lambda s=s: self._launch_sweep(s, G)).replay()
            else:
                self._launch_sweep(s, G)
            self._mark_consumed(s)
            k["h"].copy_(k["d"], non_blocking=True)
            torch.cuda.current_stream().synchronize()          # the one host wait of a batch
            r = k["h"].numpy()
            best.append(r[:G * bs].reshape(G, bs)[:, :n].copy())
            dist.append(r[G * bs:2 * G * bs].reshape(G, bs)[:, :n].copy())
            tlen.append(r[2 * G * bs:2 * G * bs + n].copy())
        d = np.concatenate(dist, axis=1).astype(np.int64) if dist else np.zeros((G, 0), np.int64)
        bst = np.concatenate(best, axis=1).astype(np.int64) if best else np.zeros((G, 0), np.int64)
        tl = np.concatenate(tlen) if tlen else np.zeros(0, np.int32)
        return dict(mean_scores=np.array([normalized_scores(d[g], tl)[0] for g in range(G)], dtype=np.float64), distances=d, best=bst)

    def predict_indices(self, clips, frame_lengths=None) -> List[np.ndarray]:
        """The decode per clip (greedy, or the beam's top-1; before the len < 3 fallback): equal to `TFLiteModel.predict_indices` clip by clip."""
        refuse_frame_lengths(frame_lengths, "BatchedTFLiteModel")
        res = []
        for idx, ln, _, _ in self._process(clips):
            res.extend(idx[b, :ln[b]].astype(np.int64) for b in range(idx.shape[0]))
        return res

    def __call__(self, clips, frame_lengths=None) -> List[Dict[str, np.ndarray]]:
        """`TFLiteModel.__call__` per clip: {'outputs': one-hot [n_chars, 59]} after the fallback (c13:22-24), on the host as there."""
        return [{"outputs": one_hot(apply_fallback(idx))} for idx in self.predict_indices(clips, frame_lengths)]

    def score(self, clips, targets, char_to_num: Optional[Dict[str, int]] = None, breakdown: bool = False) -> Dict[str, object]:
        """The test-set loop of c18:1-15 as one call: mean of (len(target) - Levenshtein(pred, target)) / len(target) over the clips, pred
        the wrapper's output (fallback applied).  targets: strings (encoded through char_to_num) or index sequences, one per clip.  The
        distances are computed on the device; the scores in float64 on the host from the integer distances and target lengths.
        breakdown: also align every pair on the device (ishara_edit_alignment after the same fallback) and add `report` (an ErrorReport over
        all clips), `ops` [n, 4] (matches, substitutions, deletions, insertions), `aligned` [n, L] and `inserted` [n, L + 1]."""
        enc = np.stack([encode_phrase(t, char_to_num, self.L) for t in targets]) if len(targets) else np.zeros((0, self.L), np.int32)
        n_clips = (np.asarray(clips[1]).shape[0] - 1) if (isinstance(clips, tuple) and len(clips) == 2 and np.ndim(clips[1]) == 1) else len(clips)
        if enc.shape[0] != n_clips:
            raise ValueError(f"{enc.shape[0]} targets for {n_clips} clips")
        if breakdown:
            self._breakdown_buffers()["conf"].zero_()      # on the current stream, outside the graph (a capture's warm-up leaves it as it was)
        parts = self._process(clips, enc, breakdown)
        dist = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, np.int32)
        tlen = np.concatenate([p[3] for p in parts]) if parts else np.zeros(0, np.int32)
        mean, scores = normalized_scores(dist, tlen)
        res = dict(mean_score=mean, scores=scores, distances=dist.astype(np.int64))
        if breakdown:
            L = self.L
            ops, aligned, inserted = (np.concatenate([p[k] for p in parts]) if parts else np.zeros((0, w), np.int32)
                                      for k, w in ((4, 4), (5, L), (6, L + 1)))
            conf = self._brk["conf"].cpu().numpy()   # the test set's matrix, read once
            res.update(report=ErrorReport.from_arrays(ops, aligned, inserted, conf, enc), ops=ops, aligned=aligned, inserted=inserted)
        return res
