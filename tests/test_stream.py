"""CPU: the streaming tick as StreamReference states it (ishara_amd/tflite_stream.py) against hand-written expectations -- what is stored and
what is dropped, the flags, the restart after a final, the endpoint's exact frame, local agreement at A = 2 and A = 3 -- and the host side
of StreamingTFLiteModel: packing, the staging layout, the constructor's refusals, the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

import stream_parity as P
from ishara_amd import _lib, make_config
from ishara_amd import tflite_stream as TS
from ishara_amd.model import Model
from ishara_amd.tflite_model import FALLBACK_PHRASE
from ishara_amd.tflite_stream import ENDPOINT, FINAL, FINISH, FRESH, FULL, RESET, STARTED, StreamReference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ishara_stream_append", "ishara_preprocess_sessions", "ishara_stream_agree")


def H(k, seed=0):
    return P.frames(k, seed, hand=1.0)


def Q(k, seed=0):
    return P.frames(k, seed, hand=0.0)


def same(a, b):
    """Bitwise equality (the frames hold NaNs)."""
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def n_frames(clip):
    """A decode that tells how many frames the clip had: [n] (and [] for the empty clip)."""
    return [len(clip)] if len(clip) else []


def tick1(ref, chunk, flag=0, decode=n_frames):
    rec, text = ref.tick([chunk], [flag], decode)
    return dict(bits=int(rec[0, 0]), n=int(rec[0, 1]), active=int(rec[0, 2]), idle=int(rec[0, 3]), dropped=int(rec[0, 4]), stable=int(rec[0, 5]),
                text=text[0, :rec[0, 6]].tolist(), pad=text[0, rec[0, 6]:].tolist())


# ---------------------------------------------------------------------------------------------------- append
def test_hand_present_is_the_filters_predicate():
    x = np.concatenate([H(2), Q(2), P.cancelling_frame()[None]])
    assert TS.hand_present(x).tolist() == [True, True, False, False, False]
    z = Q(1)
    z[0, 2 * 92 + 41] = 1e-30                         # the last hand column of the z block counts; the column after it does not
    assert TS.hand_present(z).tolist() == [True]
    z = Q(1)
    z[0, 42] = 1.0
    assert TS.hand_present(z).tolist() == [False]


def test_leading_silence_is_dropped_and_a_phrase_starts_at_its_first_hand_frame():
    ref = StreamReference(1, 32, 6)
    r = tick1(ref, Q(5))
    assert (r["bits"], r["n"], r["dropped"], r["text"]) == (0, 0, 5, [])
    for at in (0, 3, 6):                              # first hand frame at chunk index 0 / middle / last
        ref = StreamReference(1, 32, 6)
        chunk = Q(7, seed=at)
        chunk[at] = H(1)[0]
        r = tick1(ref, chunk)
        assert (r["n"], r["active"], r["idle"], r["dropped"]) == (7 - at, 1, 6 - at, at), at
        assert r["bits"] == FRESH | STARTED
        assert same(ref.raw[0, :7 - at], chunk[at:])
        assert ref.hand[0, :7 - at].tolist() == [1] + [0] * (6 - at)
        assert r["text"] == [7 - at] and set(r["pad"]) == {-1}


def test_a_cancelling_hand_frame_counts_as_absent():
    ref = StreamReference(1, 32, 6)
    chunk = np.stack([P.cancelling_frame(), H(1)[0], P.cancelling_frame(3)])
    r = tick1(ref, chunk)
    assert (r["n"], r["active"], r["idle"], r["dropped"]) == (2, 1, 1, 1)
    assert ref.hand[0, :2].tolist() == [1, 0]


def test_overflow_in_the_middle_of_a_chunk_finalises_and_the_next_tick_restarts():
    ref = StreamReference(1, 10, 6, min_active_frames=100)
    tick1(ref, H(7))
    sentinel = ref.raw.copy()
    chunk = H(6, seed=1)
    r = tick1(ref, chunk)                             # 3 fit, 3 are dropped
    assert (r["n"], r["active"], r["dropped"]) == (10, 10, 3)
    assert r["bits"] == FRESH | FINAL | FULL | STARTED and r["text"] == [10] and r["stable"] == 1
    assert same(ref.raw[0, 7:], chunk[:3]) and same(ref.raw[0, :7], sentinel[0, :7])
    r = tick1(ref, Q(2))                              # the final was reported once: the session is empty again, silence is dropped again
    assert (r["bits"], r["n"], r["active"], r["dropped"], r["stable"], r["text"]) == (0, 0, 0, 2, 0, [])
    r = tick1(ref, H(1))
    assert (r["bits"], r["n"]) == (FRESH | STARTED, 1)


def test_reset_and_finish_with_and_without_frames():
    ref = StreamReference(1, 32, 6, min_active_frames=100)
    tick1(ref, H(4))
    r = tick1(ref, None, FINISH)                      # FINISH without frames: the stored clip's decode, final, not fresh
    assert r["bits"] == FINAL | STARTED and r["text"] == [4] and r["stable"] == 1 and r["n"] == 4
    r = tick1(ref, H(3), FINISH)                      # restarted by itself; FINISH with frames
    assert r["bits"] == FRESH | FINAL | STARTED and r["text"] == [3] and r["n"] == 3
    r = tick1(ref, None)
    assert (r["bits"], r["n"], r["text"]) == (0, 0, [])
    tick1(ref, H(5))
    r = tick1(ref, H(2), RESET)                       # RESET with frames: the 5 are gone, the 2 start a phrase
    assert r["bits"] == FRESH | STARTED and (r["n"], r["dropped"]) == (2, 0)
    r = tick1(ref, None, RESET)                       # RESET without frames
    assert (r["bits"], r["n"], r["active"], r["text"], r["stable"]) == (0, 0, 0, [], 0)
    r = tick1(ref, None, FINISH)                      # FINISH on an empty session: the empty clip's decode, final
    assert r["bits"] == FINAL and r["text"] == []
    r = tick1(ref, H(2), RESET | FINISH)
    assert r["bits"] == FRESH | FINAL | STARTED and r["text"] == [2]


def test_endpoint_exactly_at_idle_frames_and_min_active_frames():
    ref = StreamReference(1, 64, 6, idle_frames=3, min_active_frames=4)
    tick1(ref, H(3))
    r = tick1(ref, Q(3))                              # idle == idle_frames, but active == 3: one hand frame short
    assert r["bits"] == FRESH | STARTED and (r["active"], r["idle"]) == (3, 3)
    tick1(ref, H(1))                                  # active == min_active_frames, idle back to 0
    r = tick1(ref, Q(2))
    assert r["bits"] == FRESH | STARTED and (r["active"], r["idle"]) == (4, 2)        # one frame before
    r = tick1(ref, Q(1))
    assert r["bits"] == FRESH | FINAL | ENDPOINT | STARTED and (r["active"], r["idle"], r["n"]) == (4, 3, 10)
    assert r["text"] == [10] and r["stable"] == 1
    r = tick1(ref, Q(1))                              # restarted: trailing silence of the old phrase is leading silence of the next
    assert (r["bits"], r["n"], r["dropped"]) == (0, 0, 1)
    # a waiting endpoint: the idle run completes inside one chunk with frames after it
    ref = StreamReference(1, 64, 6, idle_frames=3, min_active_frames=0)
    r = tick1(ref, np.concatenate([H(1), Q(5)]))
    assert r["bits"] == FRESH | FINAL | ENDPOINT | STARTED and (r["n"], r["idle"]) == (6, 5)


# ---------------------------------------------------------------------------------------------------- agree
def _agree_run(A, hyps, fresh=None, T=6):
    """One session fed one hand frame per fresh tick; returns per tick (stable_len, text)."""
    ref = StreamReference(1, 64, T, agree=A, min_active_frames=1000)
    out = []
    for i, h in enumerate(hyps):
        fr = True if fresh is None else fresh[i]
        rec, text = ref.tick([H(1, seed=i) if fr else None], [0], lambda clip, h=h: h)
        assert bool(rec[0, 0] & FRESH) == fr
        out.append((int(rec[0, 5]), text[0, :rec[0, 6]].tolist()))
        assert (text[0, rec[0, 6]:] == -1).all()
    return out, ref


def test_agreement_of_two():
    out, ref = _agree_run(2, [[1], [1, 2], [1, 2, 3], [1, 9, 3, 4], [1, 9, 3, 4], [1], [], [5, 6, 7, 8, 9, 10], [5, 6, 7, 8, 9, 10]])
    assert out[0] == (0, [1])                         # one hypothesis: nothing to agree with
    assert out[1] == (1, [1, 2])
    assert out[2] == (2, [1, 2, 3])
    assert out[3] == (2, [1, 2, 3, 4])                # a revision inside the committed prefix: the committed symbols stay, the tail follows
    assert out[4] == (4, [1, 2, 3, 4])                # agreeing twice on the revision does not rewrite them either: lcp 4 > 2 commits only [2:4]
    assert ref.committed[0, :4].tolist() == [1, 2, 3, 4]
    assert out[5] == (4, [1, 2, 3, 4])                # a hypothesis shorter than committed_len: just the committed part
    assert out[6] == (4, [1, 2, 3, 4])                # len = 0
    assert out[7] == (4, [1, 2, 3, 4, 9, 10])         # len = T
    assert out[8] == (6, [1, 2, 3, 4, 9, 10])         # lcp 6 > 4: committed[4:6] = hyp[4:6]
    assert ref.committed[0].tolist() == [1, 2, 3, 4, 9, 10] and ref.counters[0, TS.C_CLEN] == 6


def test_agreement_of_three_and_a_waiting_session():
    hyps = [[1, 2], [1, 2], [1, 3], [1, 3], [1, 3], [1, 3, 4], [1, 3, 4], [1, 3, 4], [1, 3, 4]]
    fresh = [True, True, True, True, True, True, False, False, True]
    out, ref = _agree_run(3, hyps, fresh)
    assert [o[0] for o in out] == [0, 0, 1, 1, 2, 2, 2, 2, 2]
    assert out[2] == (1, [1, 3]) and out[4] == (2, [1, 3])
    # ticks 6 and 7 store nothing: the history is not pushed, the session does not agree with itself ([1,3,4] was seen once, not three times)
    assert out[7] == (2, [1, 3, 4]) and ref.counters[0, TS.C_NHIST] == 3
    assert ref.hist_len[0].tolist() == [2, 3, 3] and ref.hist[0, :, :3].tolist() == [[1, 3, -1], [1, 3, 4], [1, 3, 4]]
    out, _ = _agree_run(3, [[7, 8]] * 3 + [[7, 8, 9]] * 3)
    assert [o[0] for o in out] == [0, 0, 2, 2, 2, 3]


def test_a_final_reports_the_hypothesis_not_the_committed_text():
    ref = StreamReference(1, 64, 6, agree=2, min_active_frames=1000)
    for i, h in enumerate([[1, 2, 3], [1, 2, 3]]):
        ref.tick([H(1, seed=i)], [0], lambda clip, h=h: h)
    rec, text = ref.tick([H(1, seed=9)], [FINISH], lambda clip: [4, 5])
    assert rec[0, 0] == FRESH | FINAL | STARTED and rec[0, 5] == 2 and text[0, :2].tolist() == [4, 5] and (text[0, 2:] == -1).all()
    assert ref.counters[0, TS.C_DONE] == 1
    rec, text = ref.tick([None], [0], lambda clip: [])
    assert rec[0].tolist() == [0] * 8 and ref.counters[0].tolist() == [0] * 8


def test_the_scenarios_exercise_what_the_gpu_tests_count():
    for A in (2, 3, 4):
        _, stats = P.run_agree(P.new_agree_reference(A), P.agree_ticks())
        print(A, stats)
        assert stats["sessions_grew"] >= 4 and stats["retractions"] > 0 and stats["non_fresh"] > 0
    snaps = P.run_append(P.new_append_reference(), P.append_ticks())
    c = np.stack([s["counters"] for s in snaps])
    assert (c[:, :, 0] == P.APPEND["window"]).any() and (c[:, :, 3] > 0).any() and c[0, 4, 1] == 0 and c[0, 0, 3] == 270


# ---------------------------------------------------------------------------------------------------- host side
def test_pack_push_and_staging_layout():
    S, mp = 4, 5
    flags_at, frames_at, total = TS.staging_layout(S, mp)
    assert flags_at % 256 == 0 and frames_at % 256 == 0 and flags_at >= (S + 1) * 8 and frames_at >= flags_at + S * 4
    assert total == frames_at + S * mp * 276 * 4
    off, flags, raw = np.full(S + 1, -1, np.int64), np.full(S, -1, np.int32), np.full((S * mp, 276), np.inf, np.float32)
    a, b = H(3), H(5, seed=1)
    rows = TS.pack_push({2: a, 0: b}, finish=[1, 2], reset=[2], sessions=S, max_push=mp, offsets=off, flags=flags, raw=raw)
    assert rows == 8 and off.tolist() == [0, 5, 5, 8, 8] and flags.tolist() == [0, FINISH, FINISH | RESET, 0]
    assert same(raw[:5], b) and same(raw[5:8], a) and np.isinf(raw[8:]).all()
    rows = TS.pack_push([None, a], (), (), S, mp, off, flags, raw)         # a short list: the sessions left out get no frames
    assert rows == 3 and off.tolist() == [0, 0, 3, 3, 3] and not flags.any()
    assert TS.pack_push({}, (), (), S, mp, off, flags, raw) == 0 and not off.any()
    with pytest.raises(ValueError, match="max_push"):
        TS.pack_push({0: H(6)}, (), (), S, mp, off, flags, raw)
    with pytest.raises(ValueError, match="276"):
        TS.pack_push({0: np.zeros((2, 275))}, (), (), S, mp, off, flags, raw)
    for bad in (dict(frames={4: a}), dict(frames={-1: a}), dict(frames=[a] * 5), dict(frames={}, finish=[4]), dict(frames={}, reset=[-1])):
        with pytest.raises(ValueError):
            TS.pack_push(bad["frames"], bad.get("finish", ()), bad.get("reset", ()), S, mp, off, flags, raw)


def test_results_and_outputs():
    rec = np.array([[FRESH | STARTED, 9, 7, 2, 3, 2, 4, 0], [FINAL | FULL | ENDPOINT, 5, 5, 0, 0, 1, 1, 0]], np.int32)
    text = np.array([[4, 5, 6, 7, -1], [8, -1, -1, -1, -1]], np.int32)
    a, b = TS.results_from(rec, text)
    assert a.session == 0 and a.text.dtype == np.int64 and a.text.tolist() == [4, 5, 6, 7] and a.stable_len == 2
    assert (a.final, a.endpoint, a.full, a.fresh, a.started, a.n_frames, a.dropped) == (False, False, False, True, True, 9, 3)
    assert (b.final, b.endpoint, b.full, b.fresh, b.started) == (True, True, True, False, False) and b.text.tolist() == [8]
    assert TS.StreamResult._fields == ("session", "text", "stable_len", "final", "endpoint", "full", "fresh", "started", "n_frames", "dropped")
    oh = TS.StreamingTFLiteModel.outputs(a)["outputs"]
    assert oh.shape == (4, 59) and oh[0, 4] == 1 and oh.sum() == 4
    assert TS.StreamingTFLiteModel.outputs(b)["outputs"].shape == (len(FALLBACK_PHRASE), 59)      # shorter than 3: the wrapper's phrase


def test_constructor_checks_without_a_device():
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276), max_batch=4), device=None)
    for kw, what in ((dict(sessions=8), "sessions"), (dict(sessions=0), "sessions"), (dict(sessions=4, window=9000), "window"),
                     (dict(sessions=4, window=0), "window"), (dict(sessions=4, max_push=0), "max_push"), (dict(sessions=4, agree=1), "agree"),
                     (dict(sessions=4, agree=5), "agree"), (dict(sessions=4, idle_frames=0), "idle_frames"),
                     (dict(sessions=4, min_active_frames=-1), "min_active_frames"), (dict(sessions=4), "no device")):
        with pytest.raises(ValueError, match=what):
            TS.StreamingTFLiteModel(m, **kw)
    wrong_f = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 224), max_batch=4), device=None)
    with pytest.raises(ValueError, match="276"):
        TS.StreamingTFLiteModel(wrong_f, sessions=4)


def test_exported_from_the_package_and_the_abi():
    import ishara_amd
    assert ishara_amd.StreamingTFLiteModel is TS.StreamingTFLiteModel and ishara_amd.StreamReference is StreamReference
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ishara_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    body = re.search(r"typedef struct ishara_stream_state \{(.*?)\} ishara_stream_state;", hdr, re.S).group(1)
    fields = [f.strip(" *") for decl in re.findall(r"[a-z0-9_]+\*? ([^;]+);", body) for f in decl.split(",")]
    assert fields == [f[0] for f in _lib.StreamState._fields_]
    for name, value in (("COUNTERS", TS.N_CNT), ("RECORD", TS.N_REC), ("RESET", RESET), ("FINISH", FINISH), ("FRESH", FRESH), ("FINAL", FINAL),
                        ("FULL", FULL), ("ENDPOINT", ENDPOINT), ("STARTED", STARTED)):
        assert int(re.search(rf"#define ISHARA_STREAM_{name} (\d+)", hdr).group(1)) == value, name
