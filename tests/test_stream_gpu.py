"""GPU: streaming recognition (ishara_amd/csrc/stream.hip, ishara_amd/tflite_stream.py).

Every integer the three kernels write equals StreamReference after every tick of the scenarios of stream_parity.py (whose comparison
test_stream_mutants.py proves sharp); ishara_preprocess_sessions is bit-identical to ishara_preprocess session by session, with and without
the hand bytes; StreamingTFLiteModel's logits are bit-equal to BatchedTFLiteModel on each session's stored frames after every tick, its
results equal the reference driven by those decodes, a final's text is the offline decode; hipGraph replay equals eager execution."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stream_parity as P
from ishara_amd import _lib, get_model
from ishara_amd import tflite_stream as TS
from ishara_amd.tflite_batch import BatchedTFLiteModel
from ishara_amd.tflite_stream import FINISH, StreamingTFLiteModel, StreamReference

pytestmark = pytest.mark.gpu

SMALL = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _stats(seed=3):
    from oracle import preprocess_oracle as PO
    g = np.random.default_rng(seed)
    return {n: (0.1 * g.standard_normal((c, 3)).astype(np.float32), (0.5 + g.random((c, 3))).astype(np.float32)) for n, c in PO.PARTS}


def _mean_std(stats):
    from oracle import preprocess_oracle as PO
    mean = torch.from_numpy(np.concatenate([stats[p][0].reshape(-1) for p, _ in PO.PARTS])).cuda()
    std = torch.from_numpy(np.concatenate([stats[p][1].reshape(-1) for p, _ in PO.PARTS])).cuda()
    return mean, std


class DeviceState:
    """The caller-owned arrays of ishara_stream_state, started from a reference's arrays."""

    def __init__(self, ref):
        self.arrays = {k: torch.from_numpy(getattr(ref, k).copy()).cuda() for k in ("raw", "hand", "counters", "hist", "hist_len", "committed")}
        self.st = _lib.StreamState(**{k: v.data_ptr() for k, v in self.arrays.items()}, S=ref.S, window=ref.window, T=ref.T, agree=ref.A)
        self.S = ref.S
        self.fresh = torch.full((ref.S,), -7, dtype=torch.int32, device="cuda")

    def host(self, name):
        return self.arrays[name].cpu().numpy()

    def append(self, lib, chunks, flags):
        rows = [np.asarray(c, np.float32).reshape(-1, 276) for c in chunks]
        off = np.zeros(self.S + 1, np.int64)
        off[1:] = np.cumsum([r.shape[0] for r in rows])
        packed = torch.from_numpy(np.concatenate(rows)).cuda() if off[-1] else None
        d_off, d_flags = torch.from_numpy(off).cuda(), torch.from_numpy(np.asarray(flags, np.int32)).cuda()
        _lib.check(lib.ishara_stream_append(C.byref(self.st), _lib.ptr(packed), int(off[-1]), _lib.ptr(d_off), _lib.ptr(d_flags), _lib.ptr(self.fresh),
                                            _stream()), "ishara_stream_append")
        return d_flags


# ------------------------------------------------------------------------------------------------ 1. append
def test_append_equals_the_frame_by_frame_loop(lib):
    ticks = P.append_ticks()
    want = P.run_append(P.new_append_reference(), ticks)
    dev = DeviceState(P.new_append_reference())            # rows and hand bytes pre-filled with the sentinel
    got = []
    for chunks, flags in ticks:
        dev.append(lib, chunks, flags)
        got.append(P.append_snapshot(dev.host("raw"), dev.host("hand"), dev.host("counters"), dev.fresh.cpu().numpy()))
    bad = P.mismatches(got, want)
    assert not bad, f"(tick, array) that differ from StreamReference: {bad[:8]}"
    last = got[-1]
    for s in range(dev.S):                                 # rows at and past n keep the pre-fill (later ticks: what a reset left, as in the reference)
        n = int(got[0]["counters"][s, 0])
        assert (got[0]["raw"][s, n:] == P.SENTINEL).all() and (got[0]["hand"][s, n:] == 0xEE).all(), s
    # deterministic: the same ticks on a second state give the same bits
    dev2 = DeviceState(P.new_append_reference())
    for chunks, flags in ticks:
        dev2.append(lib, chunks, flags)
    assert np.array_equal(dev2.host("raw").view(np.uint32), last["raw"].view(np.uint32)) and np.array_equal(dev2.host("counters"), last["counters"])


# ------------------------------------------------------------------------------------------------ 2. preprocess_sessions
def test_preprocess_sessions_bit_identical_to_single_clip(lib):
    from oracle import preprocess_oracle as PO
    T, window = 24, 70
    lengths = [0, 1, 23, 24, 25, 47, 70]                   # with a hand in every frame 23 / 24 / 25 are the kept frames: below, at, above T
    S = len(lengths)
    stats = _stats()
    mean, std = _mean_std(stats)
    clips = [P.frames(n, 2000 + n, hand=1.0 if n in (23, 24, 25) else 0.5) for n in lengths]
    clips[6][33] = P.cancelling_frame(5)                   # an odd frame whose hand values cancel: not kept, by either route
    raw = np.full((S, window, 276), P.SENTINEL, np.float32)
    hand = np.full((S, window), 0xEE, np.uint8)            # bytes past n are not read: a kept frame past n would change the output
    counters = np.full((S, 8), 99, np.int32)
    for s, x in enumerate(clips):
        raw[s, :len(x)] = x
        hand[s, :len(x)] = TS.hand_present(x)
        counters[s, 0] = len(x)
    assert not hand[6, 33] and [int(((np.arange(n) % 2 == 0) | (hand[s, :n] != 0)).sum()) for s, n in enumerate(lengths)][2:5] == [23, 24, 25]
    d_raw, d_hand, d_cnt = torch.from_numpy(raw).cuda(), torch.from_numpy(hand).cuda(), torch.from_numpy(counters).cuda()
    d_n = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    outs = []
    for n_ptr, stride, hptr in ((d_cnt, 8, d_hand), (d_n, 1, None)):
        out = torch.full((S, T, 276), float("nan"), device="cuda")
        _lib.check(lib.ishara_preprocess_sessions(_lib.ptr(d_raw), _lib.ptr(n_ptr), stride, _lib.ptr(hptr), S, window, _lib.ptr(mean), _lib.ptr(std),
                                                  _lib.ptr(out), T, _stream()), "ishara_preprocess_sessions")
        outs.append(out.cpu().numpy())
    one_raw = torch.zeros(window, 276, device="cuda")
    nd = torch.zeros(1, dtype=torch.int32, device="cuda")
    one = torch.empty(T, 276, device="cuda")
    for s, (n, x) in enumerate(zip(lengths, clips)):
        one_raw.copy_(d_raw[s])
        nd.fill_(int(n))
        _lib.check(lib.ishara_preprocess(_lib.ptr(one_raw), _lib.ptr(nd), window, _lib.ptr(mean), _lib.ptr(std), _lib.ptr(one), T, _stream()))
        single = one.cpu().numpy()
        for got, route in zip(outs, ("hand bytes", "hand == NULL")):
            assert np.array_equal(got[s].view(np.uint32), single.view(np.uint32)), f"session {s} (n={n}, {route}) differs from ishara_preprocess"
            ref = PO.preprocess(x, T, stats)
            assert np.abs(got[s] - ref).max() <= 2e-5 * (1 + np.abs(ref).max()), f"n={n} {route}"


# ------------------------------------------------------------------------------------------------ 3. agree
@pytest.mark.parametrize("A", [2, 3, 4])
def test_agree_equals_the_reference(lib, A):
    ticks = P.agree_ticks()
    want, stats = P.run_agree(P.new_agree_reference(A), ticks)
    print(f"A={A}: {stats}")
    assert stats["sessions_grew"] >= 4 and stats["retractions"] > 0 and stats["non_fresh"] > 0, f"the scenario compares too little: {stats}"
    S, T = P.AGREE["S"], P.AGREE["T"]
    dev = DeviceState(P.new_agree_reference(A))
    record = torch.full((S, 8), -7, dtype=torch.int32, device="cuda")
    text = torch.full((S, T), -7, dtype=torch.int32, device="cuda")
    no_frames = [np.zeros((0, 276), np.float32)] * S
    got = []
    for idx, ln, fresh, flags, cnt in ticks:
        d_flags = dev.append(lib, no_frames, flags)        # step 1 (RESET, or the restart after a final); no frames in this scenario
        dev.arrays["counters"][:, :4] = torch.from_numpy(cnt).cuda()
        dev.fresh.copy_(torch.from_numpy(fresh))
        d_idx, d_len = torch.from_numpy(idx).cuda(), torch.from_numpy(ln).cuda()
        _lib.check(lib.ishara_stream_agree(C.byref(dev.st), _lib.ptr(d_idx), _lib.ptr(d_len), _lib.ptr(d_flags), _lib.ptr(dev.fresh), P.AGREE["idle_frames"],
                                           P.AGREE["min_active_frames"], _lib.ptr(record), _lib.ptr(text), _stream()), "ishara_stream_agree")
        got.append(P.agree_snapshot(record.cpu().numpy(), text.cpu().numpy(), dev.host("counters"), dev.host("hist"), dev.host("hist_len"), dev.host("committed")))
    bad = P.mismatches(got, want)
    assert not bad, f"(tick, array) that differ from StreamReference: {bad[:8]}"


# ------------------------------------------------------------------------------------------------ 4. small model end to end
@pytest.fixture(scope="module")
def small():
    os.environ["ISHARA_WS_GUARD"] = "1"
    try:
        model = get_model(**SMALL, dtype="f32", max_batch=8, seed=5)
    finally:
        del os.environ["ISHARA_WS_GUARD"]
    return model, _stats()


N_TICKS, MAX_PUSH = 14, 256


def _e2e_ticks():
    """Eight clips pushed in random chunks over 12 ticks, two ticks without frames behind them: session 0 (600 frames) fills the window of
    512, 1 ends by a run of hand-less frames, 2 is finished by flag, 3 is all leading silence, 4 gets nothing, 5..7 are ordinary."""
    g = np.random.default_rng(12)
    clips = [P.frames(600, 1, 0.5), np.concatenate([P.frames(100, 2, 0.5), P.frames(40, 3, 0.0)]), P.frames(200, 4, 0.5), P.frames(300, 5, 0.0),
             P.frames(0, 6), P.frames(333, 7, 0.5), P.frames(47, 8, 0.5), P.frames(401, 9, 0.5)]
    parts = []
    for x in clips:
        cuts = np.sort(g.integers(0, len(x) + 1, 11))
        parts.append(np.split(x, cuts))
    ticks = []
    for t in range(N_TICKS):
        chunks = {s: parts[s][t] for s in range(8) if t < 12 and len(parts[s][t])}
        assert all(len(c) <= MAX_PUSH for c in chunks.values())
        ticks.append((chunks, [2] if t == 12 else []))
    return ticks


def _run_e2e(model, stats, beam_width, use_graph=True):
    """Drive a StreamingTFLiteModel and, beside it, StreamReference + BatchedTFLiteModel; returns per tick (results, logits)."""
    kw = dict(beam_width=beam_width)
    stream = StreamingTFLiteModel(model, stats=stats, sessions=8, window=512, max_push=MAX_PUSH, use_graph=use_graph, **kw)
    batched = BatchedTFLiteModel(model, stats=stats, batch_size=8, max_frames=512, use_graph=True, **kw)
    ref = StreamReference(8, 512, model.T)
    seen = dict(full=0, endpoint=0, by_flag=0, finals=0)
    out = []
    for t, (chunks, finish) in enumerate(_e2e_ticks()):
        res = stream.push(chunks, finish=finish)
        logits = stream._logits.cpu().numpy().copy()
        flags = [FINISH if s in finish else 0 for s in range(8)]
        fresh = []
        for s in range(8):
            ref.start(s, flags[s])
            fresh.append(ref.append(s, chunks[s]) if s in chunks else False)
        stored = [ref.clip(s).copy() for s in range(8)]
        decodes = batched.predict_indices(stored)
        assert np.array_equal(logits.view(np.uint32), batched._logits.cpu().numpy().view(np.uint32)), f"tick {t}: logits differ from BatchedTFLiteModel"
        rt = [ref.agree(s, decodes[s], fresh[s], flags[s]) for s in range(8)]
        want = TS.results_from(np.stack([r for r, _ in rt]), np.stack([x for _, x in rt]))
        for s, (a, b) in enumerate(zip(res, want)):
            assert np.array_equal(a.text, b.text) and a.text.dtype == np.int64, f"tick {t} session {s}: text {a.text} != {b.text}"
            assert a[2:] == b[2:] and a.session == s, f"tick {t} session {s}: {a} != {b}"
            if a.final:
                assert np.array_equal(a.text, decodes[s]) and a.stable_len == len(decodes[s]), f"tick {t} session {s}: a final is the offline decode"
                seen["finals"] += 1
                seen["full"] += a.full
                seen["endpoint"] += a.endpoint and not a.full
                seen["by_flag"] += s in finish and not a.full and not a.endpoint
        for k in ("counters", "hand", "hist", "hist_len", "committed"):
            assert np.array_equal(getattr(stream, "_" + k).cpu().numpy(), getattr(ref, k)), f"tick {t}: state array {k}"
        assert np.array_equal(stream._raw.cpu().numpy().view(np.uint32), ref.raw.view(np.uint32)), f"tick {t}: stored rows"
        out.append((res, logits))
    assert seen["full"] >= 1 and seen["endpoint"] >= 1 and seen["by_flag"] >= 1, seen
    assert not res[3].started and res[3].dropped == 300 and res[3].n_frames == 0, "session 3 is all leading silence"
    assert max(r[0].n_frames for r, _ in out) == 512
    _lib.check(model._lib.ishara_workspace_guard_check(model._h), "workspace guard")
    return out


@pytest.mark.parametrize("beam_width", [0, 4], ids=["greedy", "beam4"])
def test_small_model_streaming_equals_batched_and_the_reference(small, beam_width):
    model, stats = small
    _run_e2e(model, stats, beam_width)


def test_graph_replay_equals_eager(small):
    model, stats = small
    g = StreamingTFLiteModel(model, stats=stats, sessions=8, window=512, max_push=MAX_PUSH, use_graph=True)
    e = StreamingTFLiteModel(model, stats=stats, sessions=8, window=512, max_push=MAX_PUSH, use_graph=False)
    assert g._graph is not None and e._graph is None
    for t, (chunks, finish) in enumerate(_e2e_ticks()):
        rg = g.push(chunks, finish=finish)
        lg = g._logits.cpu().numpy().copy()
        re_ = e.push(chunks, finish=finish)
        assert np.array_equal(lg.view(np.uint32), e._logits.cpu().numpy().view(np.uint32)), f"tick {t}: hipGraph replay differs from the eager launch sequence"
        for a, b in zip(rg, re_):
            assert np.array_equal(a.text, b.text) and a[2:] == b[2:], f"tick {t}: {a} != {b}"
        for k in ("_raw", "_hand", "_counters", "_hist", "_hist_len", "_committed"):
            assert torch.equal(getattr(g, k).view(torch.uint8), getattr(e, k).view(torch.uint8)), f"tick {t}: {k}"
    _lib.check(model._lib.ishara_workspace_guard_check(model._h), "workspace guard")


def test_reset_returns_every_session_to_the_empty_record(small):
    model, stats = small
    m = StreamingTFLiteModel(model, stats=stats, sessions=8, window=512, max_push=MAX_PUSH)
    empty = m.push({})                                     # the record of eight empty sessions (text: the empty clip's decode)
    assert all(r[2:] == (0, False, False, False, False, False, 0, 0) for r in empty)
    m.push({s: P.frames(40 + s, 60 + s, 0.7) for s in range(8)})
    busy = m.push({s: P.frames(9, 80 + s, 0.7) for s in range(8)})
    assert all(r.started and r.n_frames > 9 for r in busy)
    m.reset([2, 5])
    part = m.push({})
    for s, (a, b) in enumerate(zip(part, empty)):
        if s in (2, 5):
            assert np.array_equal(a.text, b.text) and a[2:] == b[2:], s
        else:
            assert a.started and a.n_frames == busy[s].n_frames and not a.fresh, s
    m.reset()
    for a, b in zip(m.push({}), empty):
        assert np.array_equal(a.text, b.text) and a[2:] == b[2:]
    for k in ("_raw", "_hand", "_counters", "_hist", "_hist_len", "_committed"):
        assert not getattr(m, k).view(torch.uint8).any(), k
    with pytest.raises(ValueError, match="max_push"):
        m.push({0: P.frames(MAX_PUSH + 1, 1)})
