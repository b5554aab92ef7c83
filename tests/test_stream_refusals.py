"""CPU: the three streaming entry points refuse, with a message of their own and before any HIP call, a null state, S / window / T / agree
out of range, null or misaligned buffers, idle_frames < 1 and min_active_frames < 0 (all device pointers and the stream are NULL or made-up
addresses here: a call that got as far as a launch would fail with a HIP error instead, or fault).  S == 0 is a no-op."""
import ctypes as C

import pytest

from ishara_amd import _lib

N = None
A16 = 4096                  # made-up 16-byte aligned addresses: never dereferenced by a call that refuses


def _state(**kw):
    v = dict(raw=A16, hand=A16, counters=A16, hist=A16, hist_len=A16, committed=A16, S=4, window=70, T=24, agree=2)
    v.update(kw)
    return _lib.StreamState(**v)


def _append(lib, st, frames=A16, n_total=8, offsets=A16, flags=A16, fresh=A16):
    return lib.ishara_stream_append(C.byref(st) if st is not None else None, frames, n_total, offsets, flags, fresh, N)


def _agree(lib, st, idx=A16, ln=A16, flags=A16, fresh=A16, idle=15, min_active=8, record=A16, text=A16):
    return lib.ishara_stream_agree(C.byref(st) if st is not None else None, idx, ln, flags, fresh, idle, min_active, record, text, N)


def _sessions(lib, raw=A16, n=A16, stride=8, hand=A16, S=4, window=70, mean=A16, std=A16, out=A16, T=24):
    return lib.ishara_preprocess_sessions(raw, n, stride, hand, S, window, mean, std, out, T, N)


def _refused(lib, rc, *words):
    msg = lib.ishara_last_error()
    assert rc != 0, "accepted"
    assert msg and all(w.encode() in msg for w in words), msg


BAD_STATE = [(dict(S=-1), "S=-1"), (dict(window=0), "window 0"), (dict(window=8193), "window 8193"), (dict(T=0), "T=0"), (dict(T=4097), "T=4097"),
             (dict(agree=1), "agree=1"), (dict(agree=5), "agree=5"), (dict(raw=0), "null"), (dict(hand=0), "null"), (dict(counters=0), "null"),
             (dict(hist=0), "null"), (dict(hist_len=0), "null"), (dict(committed=0), "null"), (dict(raw=A16 + 4), "16-byte"),
             (dict(counters=A16 + 2), "4-byte"), (dict(hist=A16 + 1), "4-byte"), (dict(committed=A16 + 3), "4-byte")]


@pytest.mark.parametrize("kw,word", BAD_STATE, ids=[w.replace(" ", "_") + "_" + next(iter(k)) for k, w in BAD_STATE])
def test_both_state_calls_refuse_a_bad_state(lib, kw, word):
    _refused(lib, _append(lib, _state(**kw)), "ishara_stream_append", word)
    _refused(lib, _agree(lib, _state(**kw)), "ishara_stream_agree", word)


def test_append_refusals(lib):
    _refused(lib, _append(lib, None), "ishara_stream_append", "null state")
    _refused(lib, _append(lib, _state(), n_total=-1), "n_total")
    for kw in (dict(frames=N), dict(offsets=N), dict(flags=N), dict(fresh=N)):
        _refused(lib, _append(lib, _state(), **kw), "ishara_stream_append", "null")
    _refused(lib, _append(lib, _state(), frames=A16 + 4), "frames", "16-byte")
    _refused(lib, _append(lib, _state(), offsets=A16 + 4), "offsets", "8-byte")
    _refused(lib, _append(lib, _state(), flags=A16 + 2), "4-byte")
    _refused(lib, _append(lib, _state(), fresh=A16 + 1), "4-byte")
    assert _append(lib, _state(S=0, raw=0, hand=0, counters=0, hist=0, hist_len=0, committed=0), N, 0, N, N, N) == 0      # no sessions: a no-op
    _refused(lib, _append(lib, _state(S=0, agree=7), N, 0, N, N, N), "agree=7")                                            # but still checked


def test_agree_refusals(lib):
    _refused(lib, _agree(lib, None), "ishara_stream_agree", "null state")
    _refused(lib, _agree(lib, _state(), idle=0), "idle_frames 0")
    _refused(lib, _agree(lib, _state(), idle=-3), "idle_frames -3")
    _refused(lib, _agree(lib, _state(), min_active=-1), "min_active_frames -1")
    for kw in (dict(idx=N), dict(ln=N), dict(flags=N), dict(fresh=N), dict(record=N), dict(text=N)):
        _refused(lib, _agree(lib, _state(), **kw), "ishara_stream_agree", "null")
    for kw in (dict(idx=A16 + 2), dict(ln=A16 + 1), dict(record=A16 + 2), dict(text=A16 + 3)):
        _refused(lib, _agree(lib, _state(), **kw), "ishara_stream_agree", "4-byte")
    assert _agree(lib, _state(S=0), N, N, N, N, 15, 8, N, N) == 0
    _refused(lib, _agree(lib, _state(S=0), N, N, N, N, 0, 8, N, N), "idle_frames")


def test_preprocess_sessions_refusals(lib):
    for kw, word in ((dict(window=0), "window 0"), (dict(window=8193), "window 8193"), (dict(S=-1), "S=-1"), (dict(S=65536), "S=65536"),
                     (dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(stride=0), "n_stride 0"), (dict(raw=N), "null"), (dict(n=N), "null"),
                     (dict(mean=N), "null"), (dict(std=N), "null"), (dict(out=N), "null"), (dict(raw=A16 + 4), "16-byte"), (dict(out=A16 + 8), "16-byte"),
                     (dict(n=A16 + 2), "4-byte")):
        _refused(lib, _sessions(lib, **kw), "ishara_preprocess_sessions", word)
    assert _sessions(lib, raw=N, n=N, hand=N, S=0, mean=N, std=N, out=N) == 0
