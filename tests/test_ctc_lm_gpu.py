"""GPU: ishara_ctc_beam_decode_lm (csrc/ctc_beam.hip, the automaton instantiations) against the table kernel bit for bit on a bigram
automaton, against the host reference ishara_amd/ctc_beam.py at orders 3 and 5, its state edges, refusals, graph capture, its
integration into Model / TFLiteModel / BatchedTFLiteModel, and its usefulness on a second-order language.  C = 60, blank 59."""
import ctypes as C

import numpy as np
import pytest
import torch

from ishara_amd import _lib, get_model
from ishara_amd.ctc_beam import CharBigramLM, prefix_beam_search
from ishara_amd.ctc_lm import CharNGramLM, LMAutomaton
from ishara_amd.evaluation import levenshtein
from ishara_amd.tflite_batch import BatchedTFLiteModel
from ishara_amd.tflite_model import TFLiteModel

pytestmark = pytest.mark.gpu

Cn, BLANK = 60, 59
SMALL = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276))
SPARE = 8                                                    # rows allocated in front of and behind every device table


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bufs(B, nbest, T):
    """Poisoned outputs: every element must be written."""
    return (torch.full((B, nbest, T), 7, dtype=torch.int32, device="cuda"), torch.full((B, nbest), 7, dtype=torch.int32, device="cuda"),
            torch.full((B, nbest), 7.0, dtype=torch.float32, device="cuda"))


def _ws(lib, B, T, W):
    return torch.empty(max(int(lib.ishara_ctc_beam_workspace_bytes(B, T, Cn, W)), 4), dtype=torch.uint8, device="cuda")


def _padded(a, fill):
    """A table on the device with SPARE rows of `fill` on either side: (owner, view of the table proper, 16-byte aligned)."""
    a = np.ascontiguousarray(a)
    full = np.full((a.shape[0] + 2 * SPARE, a.shape[1]), fill, dtype=a.dtype)
    full[SPARE:SPARE + a.shape[0]] = a
    t = torch.from_numpy(full).cuda()
    v = t[SPARE:SPARE + a.shape[0]]
    assert v.data_ptr() % 16 == 0
    return t, v


def _decode_table(lib, x, W, nbest, lm, alpha, beta, frame_len=None):
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B, T, _ = x.shape
    ws, (idx, ln, sc) = _ws(lib, B, T, W), _bufs(B, nbest, T)
    lm_d = None if lm is None else torch.from_numpy(np.asarray(lm, dtype=np.float32)).cuda()
    if frame_len is None:
        _lib.check(lib.ishara_ctc_beam_decode(_lib.ptr(x), B, T, Cn, BLANK, W, nbest, _lib.ptr(lm_d), C.c_float(alpha), C.c_float(beta),
                                              _lib.ptr(ws), _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(sc), _stream()), "ishara_ctc_beam_decode")
    else:
        fl = torch.from_numpy(np.asarray(frame_len, np.int32)).cuda()
        _lib.check(lib.ishara_ctc_beam_decode_ex(_lib.ptr(x), B, T, Cn, BLANK, W, nbest, _lib.ptr(lm_d), C.c_float(alpha), C.c_float(beta),
                                                 _lib.ptr(ws), _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(fl), _stream()),
                   "ishara_ctc_beam_decode_ex")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()


def _decode_lm(lib, x, W, nbest, logp, nxt, start, alpha, beta, frame_len=None):
    """Raw ABI call of ishara_ctc_beam_decode_lm with logp / next as arrays [S, C] (next is not validated: the edges test needs that)."""
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B, T, _ = x.shape
    ws, (idx, ln, sc) = _ws(lib, B, T, W), _bufs(B, nbest, T)
    own_p, lp = _padded(np.asarray(logp, np.float32), -3.0e4)
    own_n, nx = _padded(np.asarray(nxt, np.int32), 1 << 30)
    fl = None if frame_len is None else torch.from_numpy(np.asarray(frame_len, np.int32)).cuda()
    _lib.check(lib.ishara_ctc_beam_decode_lm(_lib.ptr(x), B, T, Cn, BLANK, W, nbest, _lib.ptr(lp), _lib.ptr(nx), lp.shape[0], int(start),
                                             C.c_float(alpha), C.c_float(beta), _lib.ptr(ws), _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(sc),
                                             _lib.ptr(fl), _stream()), "ishara_ctc_beam_decode_lm")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()


def _same_bits(a, b):
    return all(np.array_equal(p.view(np.uint32) if p.dtype == np.float32 else p, q.view(np.uint32) if q.dtype == np.float32 else q)
               for p, q in zip(a, b))


def _hyps(idx, ln, sc, b):
    return [(idx[b, n, :ln[b, n]].tolist(), float(sc[b, n])) for n in range(ln.shape[1]) if ln[b, n] >= 0]


def _confident(g, B, T, end_blank=8, sharp=6.0, noise=1.0):
    """Logits of random alignments (runs of characters and blanks), ending in blank frames (tests/test_ctc_beam_gpu.py)."""
    end_blank = min(end_blank, T)
    x = noise * g.standard_normal((B, T, Cn))
    for b in range(B):
        t = 0
        while t < T - end_blank:
            n = int(g.integers(1, 5))
            c = BLANK if g.random() < 0.4 else int(g.integers(0, BLANK))
            x[b, t:min(t + n, T - end_blank), c] += sharp
            t += n
        x[b, T - end_blank:, BLANK] += sharp
    return x.astype(np.float32)


def _bigram(seed=0):
    g = np.random.default_rng(seed)
    return CharBigramLM.fit([g.integers(0, BLANK, int(g.integers(3, 20))).tolist() for _ in range(200)], num_classes=Cn, smoothing=0.5)


def _ngram(order, seed=0, classes=20):
    """~300 random phrases over the first `classes` classes (so that contexts repeat and the deeper states are reached)."""
    g = np.random.default_rng(seed)
    return CharNGramLM.fit([g.integers(0, classes, int(g.integers(3, 20))).tolist() for _ in range(300)], order=order, num_classes=Cn)


# ------------------------------------------------------------------------------------------------ 1. the table kernel's bits
@pytest.mark.parametrize("kind", ["random", "confident"])
@pytest.mark.parametrize("W", [1, 4, 32])
@pytest.mark.parametrize("T", [1, 17, 48])
def test_bigram_automaton_gives_the_table_kernels_bits(lib, T, W, kind):
    B, nbest, alpha, beta = 8, min(W, 2), 0.4, 0.5
    g = np.random.default_rng(1000 * T + 10 * W + (kind == "confident"))
    x = (3.0 * g.standard_normal((B, T, Cn))).astype(np.float32) if kind == "random" else _confident(g, B, T)
    table = _bigram(W)
    aut = LMAutomaton.from_bigram(table)
    assert aut.num_states == Cn and aut.start == BLANK
    ragged = np.array([0, T, T + 1, max(T // 2, 1), 1, T, max(T - 1, 1), max(T // 3, 1)], np.int32)
    for fl in (None, ragged):
        want = _decode_table(lib, x, W, nbest, table, alpha, beta, fl)
        got = _decode_lm(lib, x, W, nbest, aut.logp, aut.next, aut.start, alpha, beta, fl)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))
    assert (want[1][[0, 2]] == -1).all() and np.isneginf(want[2][[0, 2]]).all()       # frame_len 0 and T + 1 are no clips


# ------------------------------------------------------------------------------------------------ 2. the host reference, orders 3 and 5
@pytest.mark.parametrize("order", [3, 5])
@pytest.mark.parametrize("W", [1, 4, 16, 32])
@pytest.mark.parametrize("T", [48, 96])
def test_parity_with_host_reference(lib, T, W, order):
    B, nbest, alpha, beta = 16, min(W, 2), 0.4, 0.5
    lm = _ngram(order)
    aut = lm.automaton()
    g = np.random.default_rng(100 * W + T + order)
    x = _confident(g, B, T, sharp=8.0, noise=1.5)
    idx, ln, sc = _decode_lm(lib, x, W, nbest, aut.logp, aut.next, aut.start, alpha, beta)
    checked = 0
    for b in range(B):
        ref, margin = prefix_beam_search(x[b], W, nbest, lm=aut, alpha=alpha, beta=beta, return_margin=True)
        got = _hyps(idx, ln, sc, b)
        assert len(got) == len(ref) == nbest
        if margin <= 1e-3:
            continue
        checked += 1
        assert [h[0] for h in got] == [r[0].tolist() for r in ref], b
        np.testing.assert_allclose([h[1] for h in got], [r[1] for r in ref], rtol=0, atol=1e-3)
    print(f"order {order} S={aut.num_states} T={T} W={W}: {checked}/{B} clips above the 1e-3 selection margin")
    assert checked >= (0.8 if W <= 4 else 0.25) * B, checked


# ------------------------------------------------------------------------------------------------ 3. state edges
def test_single_state_automaton(lib):
    lm = CharNGramLM.fit([[1, 2, 3], [2, 2]], order=1, num_classes=Cn)
    aut = lm.automaton()
    assert aut.num_states == 1 and not aut.next.any()
    x = _confident(np.random.default_rng(1), 8, 40)
    idx, ln, sc = _decode_lm(lib, x, 8, 2, aut.logp, aut.next, 0, 0.7, 0.1)
    for b in range(8):
        ref, margin = prefix_beam_search(x[b], 8, 2, lm=aut, alpha=0.7, beta=0.1, return_margin=True)
        if margin > 1e-3:
            got = _hyps(idx, ln, sc, b)
            assert [h[0] for h in got] == [r[0].tolist() for r in ref]
            np.testing.assert_allclose([h[1] for h in got], [r[1] for r in ref], rtol=0, atol=1e-3)


def test_next_outside_the_states_is_read_as_state_zero(lib):
    aut = _ngram(3, seed=3).automaton()
    S = aut.num_states
    bad, clean = aut.next.copy(), aut.next.copy()
    bad[:, 3], bad[:, 7], bad[::2, 11] = -1, S + 5, -(1 << 31)              # whole columns: every hypothesis through 3, 7 or 11 meets one
    clean[:, 3], clean[:, 7], clean[::2, 11] = 0, 0, 0
    B, T, W = 8, 48, 8
    g = np.random.default_rng(9)
    x = _confident(g, B, T, sharp=8.0, noise=1.5)
    for b in range(B):                                       # and every clip holds 3, 7 and 11, followed by characters the LM knows
        x[b, 2:4, 3] += 25.0
        x[b, 5:7, 1] += 25.0
        x[b, 9:11, 7] += 25.0
        x[b, 12:14, 2] += 25.0
        x[b, 16:18, 11] += 25.0
    idx, ln, sc = _decode_lm(lib, x, W, 2, aut.logp, bad, aut.start, 0.6, 0.2)
    checked = 0
    for b in range(B):
        ref, margin = prefix_beam_search(x[b], W, 2, lm=LMAutomaton(aut.logp, clean, aut.start), alpha=0.6, beta=0.2, return_margin=True)
        if margin <= 1e-3:
            continue
        checked += 1
        got = _hyps(idx, ln, sc, b)
        assert [h[0] for h in got] == [r[0].tolist() for r in ref], b
        assert 3 in got[0][0] and 7 in got[0][0] and 11 in got[0][0]
        np.testing.assert_allclose([h[1] for h in got], [r[1] for r in ref], rtol=0, atol=1e-3)
    assert checked >= B // 2, checked
    assert _same_bits((idx, ln, sc), _decode_lm(lib, x, W, 2, aut.logp, clean, aut.start, 0.6, 0.2))


def test_clips_without_frames_leave_the_others_alone(lib):
    aut = _ngram(3).automaton()
    B, T, W = 8, 48, 8
    x = _confident(np.random.default_rng(12), B, T)
    fl = np.array([T, 0, 17, -3, T + 1, 1, 30, T], np.int32)
    idx, ln, sc = _decode_lm(lib, x, W, 2, aut.logp, aut.next, aut.start, 0.5, 0.3, fl)
    none = [1, 3, 4]
    assert (ln[none] == -1).all() and np.isneginf(sc[none]).all() and (idx[none] == -1).all()
    keep = [b for b in range(B) if b not in none]
    sub = _decode_lm(lib, x[keep], W, 2, aut.logp, aut.next, aut.start, 0.5, 0.3, fl[keep])
    assert _same_bits((idx[keep], ln[keep], sc[keep]), sub)
    for b in keep:                                           # and a clip of n frames is the clip cut to n frames
        one = _decode_lm(lib, x[b:b + 1, :fl[b]], W, 2, aut.logp, aut.next, aut.start, 0.5, 0.3)
        assert np.array_equal(one[1][0], ln[b]) and np.array_equal(one[2][0].view(np.uint32), sc[b].view(np.uint32))
        assert all(np.array_equal(one[0][0, n, :max(ln[b, n], 0)], idx[b, n, :max(ln[b, n], 0)]) for n in range(2))


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_before_any_launch(lib):
    aut = _ngram(3).automaton()
    S, B, T = aut.num_states, 2, 8
    x = torch.zeros((B, T, Cn), device="cuda")
    own_p, lp = _padded(aut.logp, 0.0)
    own_n, nx = _padded(aut.next, 0)
    ws, (idx, ln, sc) = _ws(lib, B, T, 4), _bufs(B, 1, T)
    fl = torch.full((B + 1,), T, dtype=torch.int32, device="cuda")
    P = C.c_void_p

    def call(C_=Cn, W=4, nbest=1, T_=T, B_=B, blank=BLANK, S_=S, start=0, logp=lp.data_ptr(), nxt=nx.data_ptr(), alpha=0.5, beta=0.0,
             ws_=ws.data_ptr(), x_=x.data_ptr(), fl_=0):
        return lib.ishara_ctc_beam_decode_lm(P(x_) if x_ else None, B_, T_, C_, blank, W, nbest, P(logp) if logp else None, P(nxt) if nxt else None,
                                             S_, start, C.c_float(alpha), C.c_float(beta), P(ws_) if ws_ else None, _lib.ptr(idx), _lib.ptr(ln),
                                             _lib.ptr(sc), P(fl_) if fl_ else None, _stream())
    idx.fill_(7)
    for kw in (dict(S_=0), dict(S_=(1 << 22) + 1), dict(start=S), dict(start=-1), dict(logp=0), dict(nxt=0), dict(logp=lp.data_ptr() + 4),
               dict(nxt=nx.data_ptr() + 8), dict(C_=65), dict(C_=1, blank=0), dict(blank=Cn), dict(blank=-1), dict(W=0), dict(W=33), dict(nbest=0),
               dict(nbest=5), dict(T_=0), dict(T_=4097), dict(B_=-1), dict(alpha=float("inf")), dict(beta=float("nan")), dict(ws_=0), dict(x_=0),
               dict(ws_=ws.data_ptr() + 2), dict(fl_=fl.data_ptr() + 2)):
        assert call(**kw) != 0, kw
        assert lib.ishara_last_error(), kw
    torch.cuda.synchronize()
    assert (idx == 7).all()                                  # nothing ran
    assert call() == 0 and call(fl_=fl.data_ptr()) == 0 and call(fl_=fl.data_ptr() + 4) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. graph capture, empty batch
def test_graph_capture_and_zero_batch(lib):
    B, T, W = 8, 64, 8
    aut = _ngram(3).automaton()
    x = torch.from_numpy(_confident(np.random.default_rng(3), B, T)).cuda()
    lp, nx = torch.from_numpy(aut.logp).cuda(), torch.from_numpy(aut.next).cuda()
    ws, (idx, ln, sc) = _ws(lib, B, T, W), _bufs(B, 1, T)

    def run():
        _lib.check(lib.ishara_ctc_beam_decode_lm(_lib.ptr(x), B, T, Cn, BLANK, W, 1, _lib.ptr(lp), _lib.ptr(nx), aut.num_states, aut.start,
                                                 C.c_float(0.5), C.c_float(0.2), _lib.ptr(ws), _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(sc), None,
                                                 _stream()), "beam lm")
    run()
    torch.cuda.synchronize()
    eager = (idx.clone(), ln.clone(), sc.clone())
    idx.fill_(5)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager[0]) and torch.equal(ln, eager[1]) and torch.equal(sc.view(torch.int32), eager[2].view(torch.int32))
    assert lib.ishara_ctc_beam_decode_lm(None, 0, T, Cn, BLANK, W, 1, None, None, 1, 0, C.c_float(0.5), C.c_float(0), None, None, None, None, None,
                                         _stream()) == 0


# ------------------------------------------------------------------------------------------------ 6. integration
def _clip(n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 276)).astype(np.float32)
    x[g.random(n) < 0.3, :42] = np.nan
    return x


def test_model_beam_decode_with_an_ngram_equals_abi(monkeypatch, lib):
    monkeypatch.setenv("ISHARA_WS_GUARD", "1")
    model = get_model(**SMALL, dtype="f32", max_batch=8, seed=5)
    x = _confident(np.random.default_rng(11), 6, 176)
    lm = _ngram(3, seed=2)
    aut = lm.automaton()
    idx, ln, sc = _decode_lm(lib, x, 8, 3, aut.logp, aut.next, aut.start, 0.3, 0.1)
    for given in (lm, aut):
        got = model.beam_decode(torch.from_numpy(x), beam_width=8, nbest=3, lm=given, alpha=0.3, beta=0.1)
        for b in range(6):
            assert [(h[0].tolist(), h[1]) for h in got[b]] == _hyps(idx, ln, sc, b)
    fl = np.array([176, 90, 1, 17, 176, 50], np.int32)
    idx, ln, sc = _decode_lm(lib, x, 8, 3, aut.logp, aut.next, aut.start, 0.3, 0.1, fl)
    got = model.beam_decode(torch.from_numpy(x), beam_width=8, nbest=3, lm=lm, alpha=0.3, beta=0.1, frame_lengths=fl)
    for b in range(6):
        assert [(h[0].tolist(), h[1]) for h in got[b]] == _hyps(idx, ln, sc, b)
    _lib.check(model._lib.ishara_workspace_guard_check(model._h), "workspace guard")


def test_tflite_wrappers_with_an_ngram_and_with_a_table(monkeypatch, lib):
    monkeypatch.setenv("ISHARA_WS_GUARD", "1")
    model = get_model(**SMALL, dtype="f32", max_batch=8, seed=5)
    g = np.random.default_rng(4)
    clips = [_clip(int(n), 300 + i) for i, n in enumerate(g.integers(1, 400, 13))]
    lm = _ngram(3, seed=3)
    aut = lm.automaton()
    kw = dict(beam_width=8, lm=lm, lm_alpha=0.3, lm_beta=0.2)
    graph = BatchedTFLiteModel(model, batch_size=8, max_frames=512, use_graph=True, **kw)
    eager = BatchedTFLiteModel(model, batch_size=8, max_frames=512, use_graph=False, **kw)
    single = TFLiteModel(model, max_frames=512, **kw)
    pg, pe = graph.predict_indices(clips), eager.predict_indices(clips)
    assert all(np.array_equal(a, b) for a, b in zip(pg, pe))
    for c, p in zip(clips, pg):
        assert np.array_equal(single.predict_indices(c), p)
    # the runner's decode is the raw entry point on the logits the runner computed (one batch of 8)
    first = graph.predict_indices(clips[:8])
    idx, ln, _ = _decode_lm(lib, graph._logits.cpu().numpy(), 8, 1, aut.logp, aut.next, aut.start, 0.3, 0.2)
    assert all(np.array_equal(first[b], idx[b, 0, :ln[b, 0]]) for b in range(8))
    # a CharBigramLM through the same constructors: the table entry point's output, as before
    table = _bigram(3)
    kt = dict(beam_width=8, lm=table, lm_alpha=0.3, lm_beta=0.2)
    tb = BatchedTFLiteModel(model, batch_size=8, max_frames=512, use_graph=True, **kt)
    first = tb.predict_indices(clips[:8])
    idx, ln, _ = _decode_table(lib, tb._logits.cpu().numpy(), 8, 1, table, 0.3, 0.2)
    assert all(np.array_equal(first[b], idx[b, 0, :ln[b, 0]]) for b in range(8))
    ts = TFLiteModel(model, max_frames=512, **kt)
    ta = BatchedTFLiteModel(model, batch_size=8, max_frames=512, beam_width=8, lm=LMAutomaton.from_bigram(table), lm_alpha=0.3, lm_beta=0.2)
    for c, p, q in zip(clips, tb.predict_indices(clips), ta.predict_indices(clips)):
        assert np.array_equal(ts.predict_indices(c), p) and np.array_equal(p, q)
    _lib.check(model._lib.ishara_workspace_guard_check(model._h), "workspace guard")


# ------------------------------------------------------------------------------------------------ 7. usefulness
def _second_order_language(seed, k=12):
    """Every character b has 4 plausible successors; the pair (a, b) before it picks 2 of them (p = 0.65 / 0.30, any character 0.05)."""
    g = np.random.default_rng(seed)
    ctx = list(range(k)) + [-1]
    subset = {b: g.choice(k, 4, replace=False) for b in ctx}
    succ = {(a, b): g.choice(subset[b], 2, replace=False) for a in ctx for b in ctx}

    def draw(max_len=20):
        out, a, b = [], -1, -1
        while len(out) < max_len:
            r = g.random()
            if r < 0.08 and len(out) >= 3:
                break
            s = succ[(a, b)]
            c = int(s[0]) if r < 0.65 else (int(s[1]) if r < 0.95 else int(g.integers(0, k)))
            out.append(c)
            a, b = b, c
        return out
    return g, k, succ, subset, draw


def _noisy_clips():
    """(logits [64, 192, C], the 64 true phrases, 2000 training phrases of the same language)."""
    g, k, succ, subset, draw = _second_order_language(2024)
    train = [draw() for _ in range(2000)]
    phrases = [draw() for _ in range(64)]
    B, T = len(phrases), 192
    x = 0.6 * g.standard_normal((B, T, Cn))
    for b, p in enumerate(phrases):
        x[b, 0, BLANK] += 5.0
        t, a2, b2 = 1, -1, -1
        for c in p:
            n = int(g.integers(2, 4))
            x[b, t:t + n, c] += 5.0
            # the confusable class, on half the characters and louder than the truth: any of the k, or one that the previous character
            # alone makes as plausible as the truth
            other = [v for v in subset[b2] if v not in succ[(a2, b2)]]
            conf = int(g.integers(0, k)) if g.random() < 0.5 else int(g.choice(other))
            x[b, t:t + n, conf] += 5.2 * (g.random() < 0.5)
            a2, b2 = b2, c
            x[b, t + n, BLANK] += 5.0
            t += n + 1
        x[b, t:, BLANK] += 5.0
    return x.astype(np.float32), phrases, train


def test_order3_beats_order2_beats_greedy_on_a_second_order_language(lib):
    """Host reference (prefix_beam_search, W = 16, alpha = 0.8) on these 64 clips, total edit distance: greedy 346, Witten-Bell order 2
    85, order 3 54: order 3 is 36 % below order 2, so a few near-tie clips decided otherwise on the device cannot turn the order."""
    x, phrases, train = _noisy_clips()
    B, T = x.shape[:2]
    xd = torch.from_numpy(x).cuda()
    gi = torch.empty((B, T), dtype=torch.int32, device="cuda")
    gl = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(lib.ishara_greedy_decode(_lib.ptr(xd), B, T, Cn, BLANK, _lib.ptr(gi), _lib.ptr(gl), _stream()), "ishara_greedy_decode")
    gi, gl = gi.cpu().numpy(), gl.cpu().numpy()
    dist = {"greedy": sum(levenshtein(gi[b, :gl[b]].tolist(), phrases[b]) for b in range(B))}
    for order in (2, 3):
        aut = CharNGramLM.fit(train, order=order, num_classes=Cn).automaton()
        idx, ln, _ = _decode_lm(lib, x, 16, 1, aut.logp, aut.next, aut.start, 0.8, 0.0)
        dist[order] = sum(levenshtein(idx[b, 0, :ln[b, 0]].tolist(), phrases[b]) for b in range(B))
    print(f"total edit distance over {B} clips: greedy {dist['greedy']}, order 2 {dist[2]}, order 3 {dist[3]}")
    assert dist[3] < dist[2] < dist["greedy"], dist
