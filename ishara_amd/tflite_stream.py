"""Streaming counterpart of `BatchedTFLiteModel`: `sessions` concurrent signers, each recognised while the sign is being made.

The whole-clip wrappers take a finished clip.  `StreamingTFLiteModel` keeps every session's raw frames on the device and, per `push`
(one tick, typically one camera frame per session), uploads only the new frames and replays one linear hipGraph:

  staging (offsets | flags | new frames) --ishara_stream_append--> session buffers --ishara_preprocess_sessions--> x [S, T, 276]
  --ishara_forward(training=0)--> logits --ishara_greedy_decode (ishara_ctc_beam_decode top-1 with beam_width > 0)--> idx, len
  --ishara_stream_agree--> record [S, 8] | text [S, T]

one non-blocking H2D copy in front, one D2H copy of `record | text` behind, one host wait.  The encoder is not causal: every tick
re-encodes each session's whole stored clip, so a session's hypothesis equals `BatchedTFLiteModel` on the frames stored so far, and the
text of a final equals the offline decode of the phrase.  What is new is the state between ticks (include/ishara_hip.h, "streaming
sessions"): leading frames without a hand are dropped, a phrase ends by `finish`, by a full window or by `idle_frames` hand-less frames
after `min_active_frames` frames with a hand, and the prefix on which the last `agree` hypotheses agree is committed and never retracted
("local agreement").  The defaults of agree / idle_frames / min_active_frames / window are not tuned on data, and the accuracy of
partial-clip hypotheses has not been measured.

`StreamReference` is the same tick frame by frame in numpy: the exact reference for every integer the device writes.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .tflite_batch import _align, apply_fallback, one_hot
from .tflite_model import N_COLS, PARTS, _beam_launch, _beam_setup

RESET, FINISH = 1, 2                                        # flag word of a tick
FRESH, FINAL, FULL, ENDPOINT, STARTED = 1, 2, 4, 8, 16      # record[0]
N_CNT = N_REC = 8
C_N, C_ACTIVE, C_IDLE, C_DROPPED, C_DONE, C_NHIST, C_CLEN = range(7)       # counters [S, 8]
R_FLAGS, R_N, R_ACTIVE, R_IDLE, R_DROPPED, R_STABLE, R_TEXTLEN = range(7)  # record [S, 8]
_ROW_BYTES = N_COLS * 4
_HAND_COLS = [a * 92 + j for a in range(3) for j in range(42)]             # the filter's order: axis, then landmark


class StreamResult(NamedTuple):
    session: int
    text: np.ndarray           # int64 indices; text[:stable_len] will not change while the phrase lasts
    stable_len: int
    final: bool                # the phrase ended in this tick: text is the offline decode of its frames, the session restarts
    endpoint: bool
    full: bool
    fresh: bool
    started: bool
    n_frames: int
    dropped: int


def hand_present(frames: np.ndarray) -> np.ndarray:
    """The frame filter's predicate per row of frames [k, 276]: the 126 hand columns summed in float32 in the kernel's order with NaN
    read as 0, present iff the sum != 0."""
    frames = np.asarray(frames, dtype=np.float32)
    acc = np.zeros(frames.shape[0], dtype=np.float32)
    for c in _HAND_COLS:
        v = frames[:, c]
        acc = acc + np.where(np.isnan(v), np.float32(0), v)
    return acc != 0


def results_from(record: np.ndarray, text: np.ndarray) -> List[StreamResult]:
    """record [S, 8] / text [S, T] of one tick as StreamResults."""
    out = []
    for s in range(record.shape[0]):
        r = record[s]
        f = int(r[R_FLAGS])
        out.append(StreamResult(s, text[s, :int(r[R_TEXTLEN])].astype(np.int64), int(r[R_STABLE]), bool(f & FINAL), bool(f & ENDPOINT),
                                bool(f & FULL), bool(f & FRESH), bool(f & STARTED), int(r[R_N]), int(r[R_DROPPED])))
    return out


# ---------------------------------------------------------------------------------------------------- reference (numpy, no device)
class StreamReference:
    """The tick of include/ishara_hip.h ("streaming sessions") as its frame-by-frame loop.  The arrays have the device's layout and
    receive the device's writes (nothing else is touched: rows past n, unused history slots and committed[committed_len:] keep what they
    held), so they compare with array_equal against the device state."""

    def __init__(self, sessions: int, window: int, T: int, agree: int = 2, idle_frames: int = 15, min_active_frames: int = 8):
        self.S, self.window, self.T, self.A, self.idle_frames, self.min_active = sessions, window, T, agree, idle_frames, min_active_frames
        self.raw = np.zeros((sessions, window, N_COLS), np.float32)
        self.hand = np.zeros((sessions, window), np.uint8)
        self.counters = np.zeros((sessions, N_CNT), np.int32)
        self.hist = np.zeros((sessions, agree, T), np.int32)
        self.hist_len = np.zeros((sessions, agree), np.int32)
        self.committed = np.zeros((sessions, T), np.int32)

    # ---- step 1
    def start(self, s: int, flags: int) -> None:
        c = self.counters[s]
        if (flags & RESET) or c[C_DONE]:
            c[:] = 0

    # ---- step 2
    def append_frame(self, s: int, frame: np.ndarray, hand: bool) -> bool:
        """One frame in order; True when it was stored."""
        c = self.counters[s]
        if (c[C_ACTIVE] == 0 and not hand) or c[C_N] == self.window:
            c[C_DROPPED] += 1
            return False
        n = int(c[C_N])
        self.raw[s, n] = frame
        self.hand[s, n] = 1 if hand else 0
        c[C_N] += 1
        if hand:
            c[C_ACTIVE] += 1
            c[C_IDLE] = 0
        else:
            c[C_IDLE] += 1
        return True

    def append(self, s: int, chunk: np.ndarray) -> bool:
        chunk = np.asarray(chunk, dtype=np.float32).reshape(-1, N_COLS)
        fresh = False
        for frame, h in zip(chunk, hand_present(chunk)):
            fresh |= self.append_frame(s, frame, bool(h))
        return fresh

    # ---- step 4
    def push_history(self, s: int, hyp: np.ndarray) -> None:
        c, A = self.counters[s], self.A
        row = np.full(self.T, -1, np.int32)
        row[:len(hyp)] = hyp
        if c[C_NHIST] < A:
            k = int(c[C_NHIST])
            c[C_NHIST] += 1
        else:
            self.hist[s, :A - 1] = self.hist[s, 1:].copy()
            self.hist_len[s, :A - 1] = self.hist_len[s, 1:].copy()
            k = A - 1
        self.hist[s, k] = row
        self.hist_len[s, k] = len(hyp)

    def common_prefix(self, s: int) -> int:
        """Length of the longest common prefix of the `agree` hypotheses in the history."""
        l, lens = 0, self.hist_len[s]
        while l < lens.min() and (self.hist[s, :, l] == self.hist[s, 0, l]).all():
            l += 1
        return l

    def commit(self, s: int, hyp: np.ndarray, l: int) -> None:
        c = self.counters[s]
        if l > c[C_CLEN]:
            self.committed[s, c[C_CLEN]:l] = hyp[c[C_CLEN]:l]
            c[C_CLEN] = l

    def agree(self, s: int, hyp, fresh: bool, flags: int) -> Tuple[np.ndarray, np.ndarray]:
        """record [8], text [T] of session s for this tick's hypothesis."""
        c = self.counters[s]
        hyp = np.asarray(hyp, dtype=np.int32).reshape(-1)[:self.T]
        L = len(hyp)
        endpoint = bool(c[C_ACTIVE] >= self.min_active and c[C_IDLE] >= self.idle_frames)
        full = bool(c[C_N] == self.window)
        final = bool(flags & FINISH) or full or endpoint
        if fresh:
            self.push_history(s, hyp)
        if c[C_NHIST] == self.A:
            self.commit(s, hyp, self.common_prefix(s))
        text = np.full(self.T, -1, np.int32)
        clen = int(c[C_CLEN])
        if final:
            text[:L] = hyp
            stable, tlen = L, L
            c[C_DONE] = 1
        else:
            text[:clen] = self.committed[s, :clen]
            if L > clen:
                text[clen:L] = hyp[clen:]
            stable, tlen = clen, max(clen, L)
        bits = (FRESH if fresh else 0) | (FINAL if final else 0) | (FULL if full else 0) | (ENDPOINT if endpoint else 0) | (STARTED if c[C_ACTIVE] > 0 else 0)
        return np.array([bits, c[C_N], c[C_ACTIVE], c[C_IDLE], c[C_DROPPED], stable, tlen, 0], np.int32), text

    def clip(self, s: int) -> np.ndarray:
        return self.raw[s, :int(self.counters[s, C_N])]

    def tick(self, chunks: Sequence, flags: Sequence[int], decode_fn: Callable[[np.ndarray], Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
        """One tick of all sessions: chunks[s] [k, 276] (None: no frames), flags[s], decode_fn(stored clip [n, 276]) -> indices.
        Returns records [S, 8] and texts [S, T], int32."""
        records, texts = np.zeros((self.S, N_REC), np.int32), np.zeros((self.S, self.T), np.int32)
        self.fresh = np.zeros(self.S, np.int32)
        for s in range(self.S):
            self.start(s, int(flags[s]))
            fresh = self.append(s, chunks[s]) if chunks[s] is not None else False
            self.fresh[s] = fresh
            records[s], texts[s] = self.agree(s, decode_fn(self.clip(s)), fresh, int(flags[s]))
        return records, texts


# ---------------------------------------------------------------------------------------------------- host helpers (no device)
def staging_layout(sessions: int, max_push: int) -> Tuple[int, int, int]:
    """Byte offsets of the staging buffer offsets int64 [S+1] | flags int32 [S] | frames f32 [S * max_push, 276]: (flags, frames, total)."""
    flags_at = _align((sessions + 1) * 8, 256)
    frames_at = _align(flags_at + sessions * 4, 256)
    return flags_at, frames_at, frames_at + sessions * max_push * _ROW_BYTES


def pack_push(frames, finish, reset, sessions: int, max_push: int, offsets: np.ndarray, flags: np.ndarray, raw: np.ndarray) -> int:
    """Fill offsets [S+1], flags [S] and raw [S * max_push, 276] for one tick; returns the rows used.  frames: {session: [k, 276]} or a
    list indexed by session (None / missing: no frames)."""
    if isinstance(frames, dict):
        bad = [s for s in frames if not (isinstance(s, (int, np.integer)) and 0 <= s < sessions)]
        if bad:
            raise ValueError(f"sessions {bad} outside 0..{sessions - 1}")
        chunks = [frames.get(s) for s in range(sessions)]
    else:
        chunks = list(frames)
        if len(chunks) > sessions:
            raise ValueError(f"{len(chunks)} chunks for {sessions} sessions")
        chunks += [None] * (sessions - len(chunks))
    flags[:] = 0
    for name, bit, which in (("finish", FINISH, finish), ("reset", RESET, reset)):
        for s in which:
            if not 0 <= int(s) < sessions:
                raise ValueError(f"{name}: session {s} outside 0..{sessions - 1}")
            flags[int(s)] |= bit
    rows = 0
    offsets[0] = 0
    for s, c in enumerate(chunks):
        if c is not None:
            c = np.asarray(c, dtype=np.float32)
            if c.ndim != 2 or c.shape[1] != N_COLS:
                raise ValueError(f"session {s}: frames must be [k, {N_COLS}], got {c.shape}")
            if c.shape[0] > max_push:
                raise ValueError(f"session {s}: chunk of {c.shape[0]} frames exceeds max_push={max_push}")
            raw[rows:rows + c.shape[0]] = c
            rows += c.shape[0]
        offsets[s + 1] = rows
    return rows


# ---------------------------------------------------------------------------------------------------- device runner
class StreamingTFLiteModel:
    def __init__(self, model, stats: Optional[Dict[str, tuple]] = None, sessions: int = 16, window: int = 1024, max_push: int = 64,
                 agree: int = 2, idle_frames: int = 15, min_active_frames: int = 8, use_graph: bool = True, beam_width: int = 0, lm=None,
                 lm_alpha: float = 0.0, lm_beta: float = 0.0, mbr_nbest: int = 0, rescore_nbest: int = 0):
        """sessions: concurrent signers (one batch slot each); window: most frames of one phrase (a phrase that fills it is finalised);
        max_push: most new frames per session and tick; agree / idle_frames / min_active_frames: see the module text (untuned defaults);
        beam_width / lm / lm_alpha / lm_beta as for BatchedTFLiteModel; mbr_nbest and rescore_nbest are refused (see below)."""
        if mbr_nbest:
            raise ValueError("StreamingTFLiteModel: mbr_nbest is refused: the stable prefix is what successive decodes of ONE decoder agree on, and the "
                             "minimum-Bayes-risk choice may jump between hypotheses from tick to tick; use BatchedTFLiteModel(mbr_nbest=) on whole clips")
        if rescore_nbest:
            raise ValueError("StreamingTFLiteModel: rescore_nbest is refused: the stable prefix is what successive decodes of ONE decoder agree on, and the "
                             "rescored top of an n-best list may jump between hypotheses from tick to tick; use BatchedTFLiteModel(rescore_nbest=) on whole clips")
        if model.F != N_COLS:
            raise ValueError(f"the TFLite wrapper feeds {N_COLS} columns (92 landmarks x 3); model has F={model.F}")
        if sessions < 1 or sessions > model.max_batch:
            raise ValueError(f"sessions {sessions} outside 1..max_batch={model.max_batch}")
        if window < 1 or window > 8192:
            raise ValueError(f"window {window} outside 1..8192")
        if max_push < 1:
            raise ValueError(f"max_push {max_push} < 1")
        if agree < 2 or agree > 4:
            raise ValueError(f"agree {agree} outside 2..4")
        if idle_frames < 1:
            raise ValueError(f"idle_frames {idle_frames} < 1")
        if min_active_frames < 0:
            raise ValueError(f"min_active_frames {min_active_frames} < 0")
        if model.device is None:
            raise ValueError("the model has no device: build it with device='cuda:N'")
        self.model, self.sessions, self.window, self.max_push, self.T = model, sessions, window, max_push, model.T
        self.agree, self.idle_frames, self.min_active_frames = agree, idle_frames, min_active_frames
        dev, S, T = model.device, sessions, model.T
        mean = np.concatenate([(stats[n][0] if stats else np.zeros((c, 3), np.float32)).reshape(-1) for n, c in PARTS])
        std = np.concatenate([(stats[n][1] if stats else np.ones((c, 3), np.float32)).reshape(-1) for n, c in PARTS])
        self._mean = torch.from_numpy(mean.astype(np.float32)).to(dev)
        self._std = torch.from_numpy(std.astype(np.float32)).to(dev)
        # session state: all-zero memory is S empty sessions
        self._raw = torch.zeros((S, window, N_COLS), dtype=torch.float32, device=dev)
        self._hand = torch.zeros((S, window), dtype=torch.uint8, device=dev)
        self._counters = torch.zeros((S, N_CNT), dtype=torch.int32, device=dev)
        self._hist = torch.zeros((S, agree, T), dtype=torch.int32, device=dev)
        self._hist_len = torch.zeros((S, agree), dtype=torch.int32, device=dev)
        self._committed = torch.zeros((S, T), dtype=torch.int32, device=dev)
        self._state = _lib.StreamState(raw=self._raw.data_ptr(), hand=self._hand.data_ptr(), counters=self._counters.data_ptr(),
                                       hist=self._hist.data_ptr(), hist_len=self._hist_len.data_ptr(), committed=self._committed.data_ptr(),
                                       S=S, window=window, T=T, agree=agree)
        # staging, the same layout on the host (pinned) and on the device
        self._flags_at, self._frames_at, nbytes = staging_layout(S, max_push)
        self._cap = S * max_push
        self._h_in = torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True)
        self._d_in = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        # results: record int32 [S, 8] | text [S, T], one D2H copy per tick
        self._d_res = torch.zeros(S * (N_REC + T), dtype=torch.int32, device=dev)
        self._h_res = torch.zeros(S * (N_REC + T), dtype=torch.int32, pin_memory=True)
        self._record, self._text = self._d_res[:S * N_REC].view(S, N_REC), self._d_res[S * N_REC:].view(S, T)
        self._fresh = torch.zeros(S, dtype=torch.int32, device=dev)
        self._x = torch.zeros((S, T, N_COLS), dtype=torch.float32, device=dev)
        self._logits = torch.zeros((S, T, model.C), dtype=torch.float32, device=dev)
        self._idx = torch.zeros((S, T), dtype=torch.int32, device=dev)
        self._len = torch.zeros(S, dtype=torch.int32, device=dev)
        self._beam = _beam_setup(model, S, beam_width, lm, lm_alpha, lm_beta)
        self._done = torch.cuda.Event()
        self.use_graph = use_graph
        self._graph = None
        if use_graph:
            self._capture()

    # ---- views of a staging buffer (host or device)
    def _off(self, buf):
        return buf[:(self.sessions + 1) * 8].view(torch.int64)

    def _flg(self, buf):
        return buf[self._flags_at:self._flags_at + self.sessions * 4].view(torch.int32)

    def _frm(self, buf):
        return buf[self._frames_at:].view(torch.float32).view(self._cap, N_COLS)

    # ---- device work of one tick: a linear chain
    def _launch(self):
        lib, m, d, S, st = self.model._lib, self.model, self._d_in, self.sessions, _lib.stream()
        ptr = _lib.ptr
        _lib.check(lib.ishara_stream_append(C.byref(self._state), ptr(self._frm(d)), self._cap, ptr(self._off(d)), ptr(self._flg(d)),
                                            ptr(self._fresh), st), "ishara_stream_append")
        _lib.check(lib.ishara_preprocess_sessions(ptr(self._raw), ptr(self._counters), N_CNT, ptr(self._hand), S, self.window, ptr(self._mean),
                                                  ptr(self._std), ptr(self._x), self.T, st), "ishara_preprocess_sessions")
        _lib.check(lib.ishara_forward(m._h, ptr(self._x), S, ptr(self._logits), 0, C.c_uint32(0), st), "ishara_forward")
        if self._beam is None:
            _lib.check(lib.ishara_greedy_decode(ptr(self._logits), S, self.T, m.C, m.C - 1, ptr(self._idx), ptr(self._len), st), "ishara_greedy_decode")
        else:
            _beam_launch(m, self._beam, self._logits, S, self._idx, self._len, st)
        _lib.check(lib.ishara_stream_agree(C.byref(self._state), ptr(self._idx), ptr(self._len), ptr(self._flg(d)), ptr(self._fresh),
                                           self.idle_frames, self.min_active_frames, ptr(self._record), ptr(self._text), st), "ishara_stream_agree")

    def _capture(self):
        """As TFLiteModel._capture.  The warm-up tick runs on empty sessions with an all-zero staging buffer (no frames, no flags): it
        stores nothing, pushes nothing and ends nothing, so the state stays S empty sessions."""
        side = torch.cuda.Stream(device=self.model.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._launch()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._launch()
        self._graph = g

    def _tick(self):
        if self._graph is not None:
            self._graph.replay()
        else:
            self._launch()

    # ---- public surface
    def push(self, frames, finish: Sequence[int] = (), reset: Sequence[int] = ()) -> List[StreamResult]:
        """One tick.  frames: {session: [k, 276] raw landmarks} or a list indexed by session, k <= max_push (sessions left out get no
        frames); finish / reset: sessions whose phrase the caller ends / discards in this tick.  Returns every session's StreamResult."""
        h, d = self._h_in, self._d_in
        rows = pack_push(frames, finish, reset, self.sessions, self.max_push, self._off(h).numpy(), self._flg(h).numpy(), self._frm(h).numpy())
        nbytes = self._frames_at + rows * _ROW_BYTES
        d[:nbytes].copy_(h[:nbytes], non_blocking=True)
        self._tick()
        self._h_res.copy_(self._d_res, non_blocking=True)
        self._done.record()
        self._done.synchronize()                     # the one host wait of a tick
        r = self._h_res.numpy()
        S = self.sessions
        return results_from(r[:S * N_REC].reshape(S, N_REC).copy(), r[S * N_REC:].reshape(S, self.T).copy())

    @staticmethod
    def outputs(result: StreamResult) -> Dict[str, np.ndarray]:
        """The TFLite-shaped output of a result (meant for a final): {'outputs': one-hot [n_chars, 59]} after the len < 3 fallback."""
        return {"outputs": one_hot(apply_fallback(np.asarray(result.text, dtype=np.int64)))}

    def reset(self, sessions: Optional[Sequence[int]] = None) -> None:
        """Zero-fill the state of the given sessions (None: all): they are empty again, nothing is reported for what they held."""
        arrays = (self._raw, self._hand, self._counters, self._hist, self._hist_len, self._committed)
        for a in arrays:
            if sessions is None:
                a.zero_()
            else:
                for s in sessions:
                    if not 0 <= int(s) < self.sessions:
                        raise ValueError(f"session {s} outside 0..{self.sessions - 1}")
                    a[int(s)].zero_()
