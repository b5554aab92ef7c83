"""GPU: ishara_ctc_beam_decode (csrc/ctc_beam.hip) against the host reference ishara_amd/ctc_beam.py at model scale, its invariants, its
integration into Model / TFLiteModel / BatchedTFLiteModel (graph capture, device scoring), and its usefulness with a bigram LM."""
import ctypes as C

import numpy as np
import pytest
import torch

from ishara_amd import _lib, get_model
from ishara_amd.ctc_beam import CharBigramLM, prefix_beam_search
from ishara_amd.evaluation import mean_score
from ishara_amd.tflite_batch import BatchedTFLiteModel
from ishara_amd.tflite_model import TFLiteModel

pytestmark = pytest.mark.gpu

CHARS = " !#$%&'()*+,-./0123456789:;=?@[_abcdefghijklmnopqrstuvwxyz~"
CHAR_TO_NUM = {c: i for i, c in enumerate(CHARS)}
Cn, BLANK = 60, 59
SMALL = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _decode(lib, x, W, nbest=1, lm=None, alpha=0.0, beta=0.0):
    """Raw ABI call: x [B, T, C] numpy -> (idx [B, nbest, T], len [B, nbest], score [B, nbest]) numpy."""
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B, T, Cc = x.shape
    ws = torch.empty(max(int(lib.ishara_ctc_beam_workspace_bytes(B, T, Cc, W)), 4), dtype=torch.uint8, device="cuda")
    idx = torch.full((B, nbest, T), 7, dtype=torch.int32, device="cuda")       # poisoned: every element must be written
    ln = torch.full((B, nbest), 7, dtype=torch.int32, device="cuda")
    sc = torch.full((B, nbest), 7.0, dtype=torch.float32, device="cuda")
    lm_d = None if lm is None else torch.from_numpy(np.asarray(lm, dtype=np.float32)).cuda()
    _lib.check(lib.ishara_ctc_beam_decode(_lib.ptr(x), B, T, Cc, Cc - 1, W, nbest, _lib.ptr(lm_d), C.c_float(alpha), C.c_float(beta),
                                          _lib.ptr(ws), _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(sc), _stream()), "ishara_ctc_beam_decode")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()


def _greedy(lib, x):
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    B, T, Cc = x.shape
    idx = torch.empty((B, T), dtype=torch.int32, device="cuda")
    ln = torch.empty(B, dtype=torch.int32, device="cuda")
    _lib.check(lib.ishara_greedy_decode(_lib.ptr(x), B, T, Cc, Cc - 1, _lib.ptr(idx), _lib.ptr(ln), _stream()), "ishara_greedy_decode")
    idx, ln = idx.cpu().numpy(), ln.cpu().numpy()
    return [idx[b, :ln[b]].tolist() for b in range(B)]


def _hyps(idx, ln, sc, b):
    return [(idx[b, n, :ln[b, n]].tolist(), float(sc[b, n])) for n in range(ln.shape[1]) if ln[b, n] >= 0]


def _confident(g, B, T, end_blank=8, sharp=6.0, noise=1.0):
    """Logits of random alignments (runs of characters and blanks), ending in blank frames."""
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
    phrases = [g.integers(0, BLANK, int(g.integers(3, 20))).tolist() for _ in range(200)]
    return CharBigramLM.fit(phrases, num_classes=Cn, smoothing=0.5)


# ------------------------------------------------------------------------------------------------ 1. parity with the host reference
@pytest.mark.parametrize("kind", ["random", "confident"])
@pytest.mark.parametrize("use_lm", [False, True], ids=["no_lm", "lm"])
@pytest.mark.parametrize("W", [1, 4, 16, 32])
def test_parity_with_host_reference(lib, W, use_lm, kind):
    B, T = 64, 384
    g = np.random.default_rng(100 * W + 10 * use_lm + (kind == "confident"))
    x = (3.0 * g.standard_normal((B, T, Cn))).astype(np.float32) if kind == "random" else _confident(g, B, T, sharp=8.0, noise=1.5)
    lm, alpha, beta = (_bigram(W), 0.4, 0.5) if use_lm else (None, 0.0, 0.0)
    nbest = min(W, 2)
    idx, ln, sc = _decode(lib, x, W, nbest, lm, alpha, beta)
    checked = 0
    for b in range(B):
        ref, margin = prefix_beam_search(x[b], W, nbest, lm=lm, alpha=alpha, beta=beta, return_margin=True)
        got = _hyps(idx, ln, sc, b)
        assert len(got) == len(ref) == nbest
        if margin <= 1e-3:
            continue
        checked += 1
        assert [h[0] for h in got] == [r[0].tolist() for r in ref], b
        np.testing.assert_allclose([h[1] for h in got], [r[1] for r in ref], rtol=0, atol=1e-3)
    print(f"W={W} lm={use_lm} {kind}: {checked}/{B} clips above the 1e-3 selection margin")
    # the margin is the smallest W-th / (W+1)-th gap over all 384 frames among ~59 W candidates: at W >= 16 near-ties deep in the beam
    # are common even on confident inputs, so 80 % is required where the beam is narrow and a lower floor where it is wide
    if kind == "confident":
        assert checked >= {1: 0.8, 4: 0.8, 16: 0.3, 32: 0.1}[W] * B, checked


@pytest.mark.parametrize("T", [6, 40])
@pytest.mark.parametrize("W", [1, 4, 16, 32])
def test_uniform_logits_pin_the_tie_order(lib, W, T):
    x = np.zeros((4, T, Cn), np.float32)
    idx, ln, sc = _decode(lib, x, W, W)
    ref = prefix_beam_search(x[0], W, W)
    for b in range(4):
        got = _hyps(idx, ln, sc, b)
        assert [h[0] for h in got] == [r[0].tolist() for r in ref]
        np.testing.assert_allclose([h[1] for h in got], [r[1] for r in ref], rtol=0, atol=1e-3)


# ------------------------------------------------------------------------------------------------ 2. invariants
def test_invariants(lib):
    B, T, W, nbest = 32, 200, 16, 16
    g = np.random.default_rng(5)
    x = np.concatenate([(2.0 * g.standard_normal((B // 2, T, Cn))).astype(np.float32), _confident(g, B // 2, T)])
    lm = _bigram(1)
    idx, ln, sc = _decode(lib, x, W, nbest, lm, 0.5, 0.2)
    for b in range(B):
        hy = _hyps(idx, ln, sc, b)
        assert len({tuple(h[0]) for h in hy}) == len(hy)                        # no duplicate prefixes
        s = [h[1] for h in hy]
        assert all(a >= c for a, c in zip(s, s[1:]))                            # scores do not increase down the list
        for n in range(nbest):
            assert (idx[b, n, max(ln[b, n], 0):] == -1).all()                    # -1 padding
    again = _decode(lib, x, W, nbest, lm, 0.5, 0.2)
    for a, c in zip((idx, ln, sc), again):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, c.view(np.uint32) if c.dtype == np.float32 else c)
    # a clip's result does not depend on its batch mates
    perm = g.permutation(B)[:7]
    sub = _decode(lib, x[perm], W, nbest, lm, 0.5, 0.2)
    for k, b in enumerate(perm):
        assert np.array_equal(sub[0][k], idx[b]) and np.array_equal(sub[1][k], ln[b])
        assert np.array_equal(sub[2][k].view(np.uint32), sc[b].view(np.uint32))


def test_unused_nbest_slots(lib):
    # C = 3, T = 2: only '', 0, 1, 01 and 10 are reachable -> 5 hypotheses in 32 slots
    x = np.random.default_rng(2).standard_normal((3, 2, 3)).astype(np.float32)
    idx, ln, sc = _decode(lib, x, 32, 32)
    for b in range(3):
        ref = prefix_beam_search(x[b], 32, 32)
        n = len(ref)
        assert n == 5
        assert (ln[b, n:] == -1).all() and np.isneginf(sc[b, n:]).all() and (idx[b, n:] == -1).all()
        assert [idx[b, k, :ln[b, k]].tolist() for k in range(n)] == [r[0].tolist() for r in ref]


def test_confident_top1_equals_greedy(lib):
    B, T = 64, 384
    x = _confident(np.random.default_rng(7), B, T, sharp=10.0, noise=0.5)
    greedy = _greedy(lib, x)
    for W in (1, 8):
        idx, ln, _ = _decode(lib, x, W)
        assert [idx[b, 0, :ln[b, 0]].tolist() for b in range(B)] == greedy


def test_graph_capture_and_zero_batch(lib):
    B, T, W = 8, 64, 8
    x = torch.from_numpy(_confident(np.random.default_rng(3), B, T)).cuda()
    ws = torch.empty(int(lib.ishara_ctc_beam_workspace_bytes(B, T, Cn, W)), dtype=torch.uint8, device="cuda")
    idx = torch.empty((B, 1, T), dtype=torch.int32, device="cuda")
    ln = torch.empty((B, 1), dtype=torch.int32, device="cuda")
    sc = torch.empty((B, 1), dtype=torch.float32, device="cuda")

    def run():
        _lib.check(lib.ishara_ctc_beam_decode(_lib.ptr(x), B, T, Cn, BLANK, W, 1, None, C.c_float(0), C.c_float(0), _lib.ptr(ws),
                                              _lib.ptr(idx), _lib.ptr(ln), _lib.ptr(sc), _stream()), "beam")
    run()
    torch.cuda.synchronize()
    eager = (idx.clone(), ln.clone(), sc.clone())
    idx.fill_(5)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(idx, eager[0]) and torch.equal(ln, eager[1]) and torch.equal(sc, eager[2])
    assert lib.ishara_ctc_beam_decode(None, 0, T, Cn, BLANK, W, 1, None, C.c_float(0), C.c_float(0), None, None, None, None, _stream()) == 0


# ------------------------------------------------------------------------------------------------ 3. integration
def _clip(n, seed):
    g = np.random.default_rng(seed)
    x = g.standard_normal((n, 276)).astype(np.float32)
    x[g.random(n) < 0.3, :42] = np.nan
    return x


def test_model_beam_decode_equals_abi(monkeypatch, lib):
    monkeypatch.setenv("ISHARA_WS_GUARD", "1")
    model = get_model(**SMALL, dtype="f32", max_batch=8, seed=5)
    x = _confident(np.random.default_rng(11), 6, 176)
    lm = _bigram(2)
    got = model.beam_decode(torch.from_numpy(x), beam_width=8, nbest=3, lm=lm, alpha=0.3, beta=0.1)
    idx, ln, sc = _decode(lib, x, 8, 3, lm, 0.3, 0.1)
    for b in range(6):
        assert [(h[0].tolist(), h[1]) for h in got[b]] == _hyps(idx, ln, sc, b)
        assert all(h[0].dtype == np.int64 for h in got[b])
    greedy = model.decode_batch(torch.from_numpy(x))                                          # greedy unchanged alongside
    assert [a.tolist() for a in greedy] == _greedy(lib, x)


def test_batched_tflite_beam_graph_eager_single_and_score(monkeypatch):
    monkeypatch.setenv("ISHARA_WS_GUARD", "1")
    model = get_model(**SMALL, dtype="f32", max_batch=8, seed=5)
    g = np.random.default_rng(4)
    clips = [_clip(int(n), 300 + i) for i, n in enumerate(g.integers(1, 400, 13))]
    lm = _bigram(3)
    kw = dict(beam_width=8, lm=lm, lm_alpha=0.3, lm_beta=0.2)
    graph = BatchedTFLiteModel(model, batch_size=8, max_frames=512, use_graph=True, **kw)
    eager = BatchedTFLiteModel(model, batch_size=8, max_frames=512, use_graph=False, **kw)
    single = TFLiteModel(model, max_frames=512, **kw)
    pg, pe = graph.predict_indices(clips), eager.predict_indices(clips)
    assert all(np.array_equal(a, b) for a, b in zip(pg, pe))
    for c, p in zip(clips, pg):
        assert np.array_equal(single.predict_indices(c), p)
    # the beam's top-1 equals the beam decoder on the logits the runner computed
    outs = graph(clips)
    num_to_char = {i: ch for ch, i in CHAR_TO_NUM.items()}
    preds = ["".join(num_to_char.get(int(s), "") for s in np.argmax(o["outputs"], axis=1)) for o in outs]
    targets = ["".join(g.choice(list(CHARS), int(k))) for k in g.integers(1, 30, 13)]
    res = graph.score(clips, targets, CHAR_TO_NUM)
    assert res["mean_score"] == mean_score(preds, targets)
    # beam_width = 0 is today's greedy runner, bit for bit
    plain = BatchedTFLiteModel(model, batch_size=8, max_frames=512)
    zero = BatchedTFLiteModel(model, batch_size=8, max_frames=512, beam_width=0)
    assert all(np.array_equal(a, b) for a, b in zip(plain.predict_indices(clips), zero.predict_indices(clips)))
    assert plain.score(clips, targets, CHAR_TO_NUM)["distances"].tolist() == zero.score(clips, targets, CHAR_TO_NUM)["distances"].tolist()
    t0 = TFLiteModel(model, max_frames=512, beam_width=0)
    tp = TFLiteModel(model, max_frames=512)
    for c in clips[:4]:
        assert np.array_equal(t0.predict_indices(c), tp.predict_indices(c))
    _lib.check(model._lib.ishara_workspace_guard_check(model._h), "workspace guard")


# ------------------------------------------------------------------------------------------------ 4. usefulness
def test_bigram_lm_beats_greedy_on_noisy_emissions(lib):
    g = np.random.default_rng(2024)
    # a peaked bigram over 12 characters: each character has two likely successors
    k = 12
    lm_true = np.full((Cn, Cn), 1e-4)
    for r in list(range(k)) + [BLANK]:
        nxt = g.choice(k, 2, replace=False)
        lm_true[r, nxt] = [0.6, 0.3]
        lm_true[r, BLANK] += 0.1 if r != BLANK else 0.0
    lm_true /= lm_true.sum(axis=1, keepdims=True)
    truth = CharBigramLM(np.log(lm_true).astype(np.float32))
    phrases = [p for p in (truth.sample(g, 20) for _ in range(400)) if len(p) >= 3][:128]
    lm = CharBigramLM.fit([p for p in (truth.sample(g, 20) for _ in range(2000)) if p], num_classes=Cn, smoothing=0.1)
    B, T = len(phrases), 192
    x = 0.6 * g.standard_normal((B, T, Cn))
    for b, p in enumerate(phrases):
        x[b, 0, BLANK] += 5.0
        t = 1
        for c in p:
            n = int(g.integers(2, 4))
            x[b, t:t + n, c] += 5.0
            x[b, t:t + n, int(g.integers(0, k))] += 4.8 * (g.random() < 0.5)      # a confusable class on half the characters
            x[b, t + n, BLANK] += 5.0
            t += n + 1
        x[b, t:, BLANK] += 5.0
    x = x.astype(np.float32)
    targets = ["".join(CHARS[c] for c in p) for p in phrases]
    greedy = ["".join(CHARS[c] for c in s) for s in _greedy(lib, x)]
    idx, ln, _ = _decode(lib, x, 16, 1, lm, 0.8, 0.0)
    beam = ["".join(CHARS[c] for c in idx[b, 0, :ln[b, 0]]) for b in range(B)]
    s_greedy, s_beam = mean_score(greedy, targets), mean_score(beam, targets)
    print(f"c18 score: greedy {s_greedy:.4f}, beam 16 + bigram {s_beam:.4f}")
    assert s_beam > s_greedy + 0.02, (s_beam, s_greedy)
