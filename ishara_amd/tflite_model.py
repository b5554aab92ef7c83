"""TFLite-shaped inference wrapper — `TFLiteModel` of conv-hybrid-model.ipynb c13:1-25 and the `serving_default`
signature the reference exports (c14, c16:10-14): input `inputs` float32 [n_frames, 276] raw landmarks with NaNs,
output {'outputs': float32 one-hot [n_chars, 59]}.

Device side (all in libishara_hip.so): preprocessing kernel (frame filter, resize/pad, normalise, NaN->0) -> encoder
forward at B=1 -> greedy decode, captured ONCE into a hipGraph (torch.cuda.CUDAGraph only records the launches the
library makes on the capture stream) and replayed per clip.  Host side: the len<3 fallback phrase and one_hot(., 59)
(c13:22-24), as in the reference wrapper.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._lib import stream as _stream
from .model import Model

N_COLS = 276
# concat order of pre_process1 (c3:111) with landmark counts
PARTS = [("lip", 40), ("rhand", 21), ("lhand", 21), ("rpose", 5), ("lpose", 5)]
FALLBACK_PHRASE = np.array([17, 0, 32, 12, 36, 0, 12, 32, 49, 46, 36], dtype=np.int64)     # c13:22-23

# MediaPipe landmark ids behind the 92 selected landmarks (dataset metadata, c1:12-22): 40 lip points of the face mesh, the arm /
# hand points of the pose model for the left (13..21 odd) and right (14..22 even) side
LIP_IDS = (61, 185, 40, 39, 37, 0, 267, 269, 270, 409, 291, 146, 91, 181, 84, 17, 314, 405, 321, 375,
           78, 191, 80, 81, 82, 13, 312, 311, 310, 415, 95, 88, 178, 87, 14, 317, 402, 318, 324, 308)
LPOSE_IDS, RPOSE_IDS = tuple(range(13, 22, 2)), tuple(range(14, 23, 2))


def selected_columns():
    """SEL_COLS of the reference (c1:24-28): the parquet column names the 276 input features are read from — one block per axis
    (x | y | z), inside a block right hand 0..20, left hand 0..20, left pose, right pose, lips."""
    per_axis = ([("right_hand", i) for i in range(21)] + [("left_hand", i) for i in range(21)]
                + [("pose", i) for i in LPOSE_IDS + RPOSE_IDS] + [("face", i) for i in LIP_IDS])
    return [f"{axis}_{part}_{i}" for axis in "xyz" for part, i in per_axis]


def write_inference_args(path: str = "inference_args.json") -> str:
    """The side file the reference ships next to `model.tflite` (c14:9-10) and reads back in c15:1-2:
    `{"selected_columns": SEL_COLS}`."""
    import json
    with open(path, "w") as f:
        json.dump({"selected_columns": selected_columns()}, f)
    return path


def refuse_frame_lengths(frame_lengths, who: str) -> None:
    """The TFLite-shaped wrappers take a raw clip and resize it to the model's frame count (c3:61-115): their reference graph has no
    padding and no mask, so Model's frame_lengths have no meaning here."""
    if frame_lengths is not None:
        raise ValueError(f"{who}: frame_lengths are refused: the wrapper resizes every clip to the model's frame count, its graph (c13:9-24) has no mask; "
                         "use Model(x, frame_lengths=) on padded batches")


class _BeamConfig:
    """Device state of a wrapper's beam decoder, allocated once at construction (graph replays reuse it)."""
    def __init__(self, width, lm_dev, alpha, beta, ws, score):
        self.width, self.lm, self.alpha, self.beta, self.ws, self.score = width, lm_dev, alpha, beta, ws, score


def _beam_setup(model: Model, batch: int, beam_width: int, lm, alpha: float, beta: float) -> Optional[_BeamConfig]:
    """None for beam_width == 0 (greedy); else the LM (a table, or an automaton's two tables), the workspace and the top-1 score buffer
    on the model's device."""
    from . import ctc_beam
    if beam_width == 0:
        if lm is not None:
            raise ValueError("an lm needs beam_width > 0")
        return None
    ctc_beam.check_device_args(model.C, model.T, beam_width, 1)
    dev = model.device
    lm_dev = ctc_beam.lm_to_device(lm, model.C, dev)
    ws = torch.empty(max(ctc_beam.workspace_bytes(model._lib, batch, model.T, model.C, beam_width), 4), dtype=torch.uint8, device=dev)
    score = torch.zeros(batch, dtype=torch.float32, device=dev)
    return _BeamConfig(int(beam_width), lm_dev, float(alpha), float(beta), ws, score)


def _beam_launch(model: Model, cfg: _BeamConfig, logits, batch: int, idx, ln, stream) -> None:
    """ishara_ctc_beam_decode with nbest = 1: idx [batch, T] / ln [batch] in the layout ishara_greedy_decode writes."""
    from . import ctc_beam
    ctc_beam.launch(model._lib, logits, batch, model.T, model.C, cfg.width, 1, cfg.lm, cfg.alpha, cfg.beta, cfg.ws, idx, ln, cfg.score, stream)


class _MbrConfig:
    """Device state of a wrapper's minimum-Bayes-risk selection (ishara_amd/mbr.py): the n-best buffers the beam search fills and the
    selection reads, the selected slots, and 1 / temperature as the device float every launch reads."""
    def __init__(self, nbest, mode, inv_temp, hyp_idx, hyp_len, hyp_score, best):
        self.nbest, self.mode, self.inv_temp, self.hyp_idx, self.hyp_len, self.hyp_score, self.best = nbest, mode, inv_temp, hyp_idx, hyp_len, hyp_score, best


def _mbr_setup(model: Model, batch: int, beam: Optional[_BeamConfig], mbr_nbest: int, temperature: float, normalise: bool) -> Optional[_MbrConfig]:
    """None for mbr_nbest == 0 (nothing is allocated); else 2 <= mbr_nbest <= beam_width and the buffers on the model's device."""
    from . import ctc_beam, mbr
    if mbr_nbest == 0:
        return None
    if mbr_nbest < 2:
        raise ValueError(f"mbr_nbest {mbr_nbest}: 0 (off) or at least 2 hypotheses to choose among")
    if beam is None or beam.width < mbr_nbest:
        raise ValueError(f"mbr_nbest {mbr_nbest} needs beam_width >= mbr_nbest, got beam_width {0 if beam is None else beam.width}")
    ctc_beam.check_device_args(model.C, model.T, beam.width, mbr_nbest)
    mode = mbr.check_device_args(mbr_nbest, model.T, model.C, 1 if normalise else 0)
    dev = model.device
    inv_temp = torch.full((1,), mbr.inverse_temperature(temperature), dtype=torch.float32, device=dev)
    return _MbrConfig(int(mbr_nbest), mode, inv_temp, torch.full((batch, mbr_nbest, model.T), -1, dtype=torch.int32, device=dev),
                      torch.full((batch, mbr_nbest), -1, dtype=torch.int32, device=dev), torch.zeros((batch, mbr_nbest), dtype=torch.float32, device=dev),
                      torch.zeros(batch, dtype=torch.int32, device=dev))


def _mbr_launch(model: Model, beam: _BeamConfig, cfg: _MbrConfig, logits, batch: int, idx, ln, stream) -> None:
    """ishara_ctc_beam_decode with nbest = cfg.nbest into cfg's buffers, then ishara_mbr_select into idx [batch, T] / ln [batch], the layout
    ishara_greedy_decode writes."""
    from . import ctc_beam, mbr
    ctc_beam.launch(model._lib, logits, batch, model.T, model.C, beam.width, cfg.nbest, beam.lm, beam.alpha, beam.beta, beam.ws, cfg.hyp_idx,
                    cfg.hyp_len, cfg.hyp_score, stream)
    mbr.launch(model._lib, cfg.hyp_idx, cfg.hyp_len, cfg.hyp_score, None, cfg.inv_temp, batch, cfg.nbest, model.T, model.C, cfg.mode, idx, ln, cfg.best,
               None, None, None, None, stream)


def _set_mbr_temperature(cfg: Optional[_MbrConfig], temperature: float) -> None:
    from . import mbr
    if cfg is None:
        raise ValueError("set_mbr_temperature: the wrapper was built without mbr_nbest")
    cfg.inv_temp.fill_(mbr.inverse_temperature(temperature))


class _RescoreConfig:
    """Device state of a wrapper's second pass (ishara_amd/rescore.py): the n-best buffers the beam search fills, the exact scores, the
    rescored list, and params = (weight, alpha, beta) / 1 / temperature as the device floats every launch reads."""
    def __init__(self, nbest, lm_dev, eos, values, params, inv_temp, batch, T, dev):
        self.nbest, self.lm, self.eos, self.params, self.inv_temp = nbest, lm_dev, eos, params, inv_temp
        self.hyp_idx = torch.full((batch, nbest, T), -1, dtype=torch.int32, device=dev)
        self.hyp_len = torch.full((batch, nbest), -1, dtype=torch.int32, device=dev)
        self.hyp_score = torch.zeros((batch, nbest), dtype=torch.float32, device=dev)
        self.logp = torch.zeros((batch, nbest), dtype=torch.float32, device=dev)
        self.out_idx = torch.full((batch, nbest, T), -1, dtype=torch.int32, device=dev)
        self.out_len = torch.full((batch, nbest), -1, dtype=torch.int32, device=dev)
        self.out_score = torch.zeros((batch, nbest), dtype=torch.float32, device=dev)
        self.posterior = torch.zeros((batch, nbest), dtype=torch.float32, device=dev)
        self.best = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.values = [float(v) for v in values]             # the host's copy of (weight, alpha, beta)
        from . import rescore
        self.ptrs = rescore.pointer_array([self.logp])


def _rescore_setup(model: Model, batch: int, beam: Optional[_BeamConfig], mbr: Optional[_MbrConfig], rescore_nbest: int, lm, alpha: float, beta: float,
                   temperature: float) -> Optional[_RescoreConfig]:
    """None for rescore_nbest == 0 (nothing is allocated); else 2 <= rescore_nbest <= beam_width, equal to mbr_nbest when that is set, and
    the buffers on the model's device."""
    import math
    from . import ctc_beam, rescore
    from . import mbr as mbr_mod
    if rescore_nbest == 0:
        if lm is not None or float(alpha) != 0.0 or float(beta) != 0.0:
            raise ValueError("rescore_lm / rescore_alpha / rescore_beta need rescore_nbest >= 2")
        return None
    if rescore_nbest < 2:
        raise ValueError(f"rescore_nbest {rescore_nbest}: 0 (off) or at least 2 hypotheses to rerank")
    if beam is None or beam.width < rescore_nbest:
        raise ValueError(f"rescore_nbest {rescore_nbest} needs beam_width >= rescore_nbest, got beam_width {0 if beam is None else beam.width}")
    if mbr is not None and mbr.nbest != rescore_nbest:
        raise ValueError(f"mbr_nbest {mbr.nbest} must equal rescore_nbest {rescore_nbest}: the vote runs over the rescored list")
    if rescore_nbest > rescore.MAX_NBEST:
        raise ValueError(f"rescore_nbest {rescore_nbest} outside 2..{rescore.MAX_NBEST}")
    if not (math.isfinite(float(alpha)) and math.isfinite(float(beta))):
        raise ValueError("rescore_alpha and rescore_beta must be finite")
    ctc_beam.check_device_args(model.C, model.T, beam.width, rescore_nbest)
    dev = model.device
    lm_dev = rescore.lm_to_device(lm, dev)
    if lm_dev is not None and int(lm_dev.logp.shape[1]) != model.C:
        raise ValueError(f"rescore_lm has {int(lm_dev.logp.shape[1])} classes, the model {model.C}")
    values = [1.0, float(alpha), float(beta)]
    params = torch.tensor(values, dtype=torch.float32, device=dev)
    inv_temp = torch.full((1,), mbr_mod.inverse_temperature(temperature), dtype=torch.float32, device=dev)
    return _RescoreConfig(int(rescore_nbest), lm_dev, model.C - 1, values, params, inv_temp, batch, model.T, dev)


def _rescore_search(model: Model, beam: _BeamConfig, cfg: _RescoreConfig, logits, batch: int, stream) -> None:
    """the n-best of the beam search into cfg's buffers and their exact CTC scores under `logits` into cfg.logp"""
    from . import ctc_beam
    ctc_beam.launch(model._lib, logits, batch, model.T, model.C, beam.width, cfg.nbest, beam.lm, beam.alpha, beam.beta, beam.ws, cfg.hyp_idx,
                    cfg.hyp_len, cfg.hyp_score, stream)
    _lib.check(model._lib.ishara_ctc_score_nbest(_lib.ptr(logits), batch, model.T, model.C, model.C - 1, _lib.ptr(cfg.hyp_idx), _lib.ptr(cfg.hyp_len),
                                                 cfg.nbest, model.T, None, _lib.ptr(cfg.logp), None, stream), "ishara_ctc_score_nbest")


def _rescore_launch(model: Model, beam: _BeamConfig, cfg: _RescoreConfig, mbr: Optional[_MbrConfig], logits, batch: int, idx, ln, stream) -> None:
    """beam search (nbest = cfg.nbest), ishara_ctc_score_nbest on `logits`, ishara_nbest_rescore_p, then the top row (or, with mbr, the
    ishara_mbr_select choice voted with the posterior) into idx [batch, T] / ln [batch], the layout ishara_greedy_decode writes."""
    from . import mbr as mbr_mod
    from . import rescore
    _rescore_search(model, beam, cfg, logits, batch, stream)
    rescore.launch_p(model._lib, cfg.hyp_idx, cfg.hyp_len, batch, cfg.nbest, model.T, cfg.ptrs, 1, cfg.params, cfg.lm, cfg.eos, cfg.inv_temp, cfg.out_idx,
                     cfg.out_len, cfg.out_score, cfg.posterior, None, stream)
    if mbr is not None:
        mbr_mod.launch(model._lib, cfg.out_idx, cfg.out_len, None, cfg.posterior, None, batch, cfg.nbest, model.T, model.C, mbr.mode, idx, ln, cfg.best,
                       None, None, None, None, stream)
    else:                                        # the top row; a clip always has a live hypothesis (the empty one at least), the clamp is for the layout
        idx.copy_(cfg.out_idx[:, 0])
        torch.clamp(cfg.out_len[:, 0], min=0, out=ln)


def _set_rescore(cfg: Optional[_RescoreConfig], weight, alpha, beta, temperature) -> None:
    import math
    from . import mbr
    if cfg is None:
        raise ValueError("set_rescore: the wrapper was built without rescore_nbest")
    vals = [cfg.values[k] if v is None else float(v) for k, v in enumerate((weight, alpha, beta))]
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("set_rescore: weight, alpha and beta must be finite")
    it = None if temperature is None else mbr.inverse_temperature(temperature)
    cfg.params.copy_(torch.tensor(vals, dtype=torch.float32))
    cfg.values = vals
    if it is not None:
        cfg.inv_temp.fill_(it)


class TFLiteModel:
    def __init__(self, model: Model, stats: Optional[Dict[str, tuple]] = None, max_frames: int = 1024, use_graph: bool = True,
                 beam_width: int = 0, lm=None, lm_alpha: float = 0.0, lm_beta: float = 0.0, mbr_nbest: int = 0, mbr_temperature: float = 1.0,
                 mbr_normalise: bool = True, rescore_nbest: int = 0, rescore_lm=None, rescore_alpha: float = 0.0, rescore_beta: float = 0.0,
                 rescore_temperature: float = 1.0):
        """beam_width = 0: the reference's greedy decode (c8:4-12).  beam_width > 0: the CTC prefix beam search of ishara_amd/ctc_beam.py
        (top-1, optional LM weighted by lm_alpha, lm_beta per character: a table lm [C, C], or a CharNGramLM / LMAutomaton of ctc_lm.py,
        whose device tables are built here once) replaces it inside the same graph.  mbr_nbest >= 2 (needs beam_width >= mbr_nbest): the
        beam search keeps mbr_nbest hypotheses and ishara_mbr_select (ishara_amd/mbr.py) picks the one of smallest expected edit distance
        under the votes exp((score - max) / mbr_temperature), normalised by the voter's length with mbr_normalise; 0 changes nothing.
        rescore_nbest >= 2 (needs beam_width >= rescore_nbest): the second pass of ishara_amd/rescore.py inside the same graph: the beam
        search (with its own lm / lm_alpha / lm_beta) keeps rescore_nbest hypotheses, ishara_ctc_score_nbest scores them exactly on the
        wrapper's logits, ishara_nbest_rescore_p reranks by logp + rescore_alpha * rescore_lm + rescore_beta * len, and the top row is
        what everything downstream reads; with mbr_nbest == rescore_nbest the ishara_mbr_select vote, weighted by the posterior at
        rescore_temperature, follows instead (Model.rescore_decode(mbr=True)).  0 allocates, launches and captures nothing new."""
        if model.F != N_COLS:
            raise ValueError(f"the TFLite wrapper feeds {N_COLS} columns (92 landmarks x 3); model has F={model.F}")
        self.model, self.max_frames, self.T = model, max_frames, model.T
        dev = model.device
        mean = np.concatenate([(stats[n][0] if stats else np.zeros((c, 3), np.float32)).reshape(-1) for n, c in PARTS])
        std = np.concatenate([(stats[n][1] if stats else np.ones((c, 3), np.float32)).reshape(-1) for n, c in PARTS])
        self._mean = torch.from_numpy(mean.astype(np.float32)).to(dev)
        self._std = torch.from_numpy(std.astype(np.float32)).to(dev)
        self._raw = torch.zeros((max_frames, N_COLS), dtype=torch.float32, device=dev)
        self._n = torch.zeros(1, dtype=torch.int32, device=dev)
        self._x = torch.zeros((1, self.T, N_COLS), dtype=torch.float32, device=dev)
        self._logits = torch.zeros((1, self.T, model.C), dtype=torch.float32, device=dev)
        self._idx = torch.zeros((1, self.T), dtype=torch.int32, device=dev)
        self._len = torch.zeros(1, dtype=torch.int32, device=dev)
        self._beam = _beam_setup(model, 1, beam_width, lm, lm_alpha, lm_beta)
        self._mbr = _mbr_setup(model, 1, self._beam, mbr_nbest, mbr_temperature, mbr_normalise)
        self._rescore = _rescore_setup(model, 1, self._beam, self._mbr, rescore_nbest, rescore_lm, rescore_alpha, rescore_beta, rescore_temperature)
        self._graph = None
        if use_graph:
            self._capture()

    def _launch(self):
        lib, m = self.model._lib, self.model
        _lib.check(lib.ishara_preprocess(_lib.ptr(self._raw), _lib.ptr(self._n), self.max_frames, _lib.ptr(self._mean), _lib.ptr(self._std),
                                         _lib.ptr(self._x), self.T, _stream()), "ishara_preprocess")
        _lib.check(lib.ishara_forward(m._h, _lib.ptr(self._x), 1, _lib.ptr(self._logits), 0, C.c_uint32(0), _stream()), "ishara_forward")
        if self._beam is None:
            _lib.check(lib.ishara_greedy_decode(_lib.ptr(self._logits), 1, self.T, m.C, m.C - 1, _lib.ptr(self._idx), _lib.ptr(self._len), _stream()),
                       "ishara_greedy_decode")
        elif self._rescore is not None:
            _rescore_launch(m, self._beam, self._rescore, self._mbr, self._logits, 1, self._idx, self._len, _stream())
        elif self._mbr is not None:
            _mbr_launch(m, self._beam, self._mbr, self._logits, 1, self._idx, self._len, _stream())
        else:
            _beam_launch(m, self._beam, self._logits, 1, self._idx, self._len, _stream())

    def set_mbr_temperature(self, temperature: float) -> None:
        """1 / temperature written into the device float every replay reads (on the current stream; no new capture)."""
        _set_mbr_temperature(self._mbr, temperature)

    def set_rescore(self, weight=None, alpha=None, beta=None, temperature=None) -> None:
        """The second pass's parameters written into the device floats every replay reads (on the current stream; no new capture): the
        weight on the exact score (1 at construction), alpha, beta, the posterior's temperature; None leaves a value as it is."""
        _set_rescore(self._rescore, weight, alpha, beta, temperature)

    def _capture(self):
        side = torch.cuda.Stream(device=self.model.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._launch()                       # warm-up outside capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._launch()
        self._graph = g

    def predict_indices(self, inputs, frame_lengths=None) -> np.ndarray:
        refuse_frame_lengths(frame_lengths, "TFLiteModel")
        x = np.asarray(inputs, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != N_COLS:
            raise ValueError(f"inputs must be [n_frames, {N_COLS}]")
        n = x.shape[0]
        if n > self.max_frames:
            raise ValueError(f"clip of {n} frames exceeds max_frames={self.max_frames}")
        if n:
            self._raw[:n].copy_(torch.from_numpy(np.ascontiguousarray(x)), non_blocking=False)
        self._n.fill_(n)
        if self._graph is not None:
            self._graph.replay()
        else:
            self._launch()
        ln = int(self._len.item())
        return self._idx[0, :ln].cpu().numpy().astype(np.int64)

    def __call__(self, inputs, frame_lengths=None) -> Dict[str, np.ndarray]:
        idx = self.predict_indices(inputs, frame_lengths)
        if idx.shape[0] < 3:                                  # c13:22-23
            idx = FALLBACK_PHRASE
        out = np.zeros((idx.shape[0], 59), dtype=np.float32)  # tf.one_hot(x, 59): index 59 -> zero row
        ok = idx < 59
        out[np.arange(idx.shape[0])[ok], idx[ok]] = 1.0
        return {"outputs": out}

    def export(self, directory: str = ".", weights: str = "model.h5") -> Dict[str, str]:
        """The export step of c14:1-10 as far as this build goes: the model's weights (`model.h5`, Keras-2 `save_weights` layout; use a
        `.npz` name where libhdf5 is missing) and `inference_args.json`.  The fp16 numerics of the reference's `.tflite` are what
        `get_model(dtype="f16")` runs; the flatbuffer container itself is not written (nothing in this image can validate one)."""
        import os
        os.makedirs(directory, exist_ok=True)
        wpath = os.path.join(directory, weights)
        self.model.save_weights(wpath)
        return {"weights": wpath, "inference_args": write_inference_args(os.path.join(directory, "inference_args.json"))}

    # reference spelling: interpreter.get_signature_runner("serving_default")(inputs=frame)  (c16:10-13)
    def get_signature_runner(self, name: str = "serving_default"):
        if name != "serving_default":
            raise KeyError(name)
        return lambda inputs: self(inputs)
