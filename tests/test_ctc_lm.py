"""CPU: the character n-gram LM of ishara_amd/ctc_lm.py (interpolated Witten-Bell, as a deterministic automaton), the host beam search
with an automaton as lm=, and the choice of the entry point."""
import numpy as np
import pytest

from ishara_amd import _lib
from ishara_amd.ctc_beam import CharBigramLM, prefix_beam_search
from ishara_amd.ctc_lm import BOS, CharNGramLM, DeviceAutomaton, LMAutomaton, as_automaton, entry_point

Cn, BLANK = 60, 59
K = 9                                                       # the phrases use few classes, so that contexts repeat


def _phrases(seed=0, n=300):
    g = np.random.default_rng(seed)
    return [g.integers(0, K, int(g.integers(1, 14))).tolist() for _ in range(n)]


def _prefixes(g, n=400):
    """Random prefixes: seen ones, ones with classes no phrase holds (unseen continuations) and ones far longer than any order."""
    out = [[]]
    for _ in range(n):
        hi = K if g.random() < 0.6 else BLANK
        out.append(g.integers(0, hi, int(g.integers(0, 13))).tolist())
    return out


def _exact(lm, aut, logp64, prefixes):
    """logp[state_after(prefix), c] == logprob(prefix, c) for every prefix and class, in fp64."""
    for p in prefixes:
        s = aut.state_after(p)
        direct = np.array([lm.logprob(p, c) for c in range(Cn)])
        if not np.array_equal(logp64[s], direct):
            return False
    return True


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5])
def test_rows_normalise_and_automaton_equals_direct_evaluation(order):
    lm = CharNGramLM.fit(_phrases(), order=order, num_classes=Cn)
    aut = lm.automaton()
    logp64 = lm.logp_fp64()
    assert aut.logp.dtype == np.float32 and aut.next.dtype == np.int32 and aut.logp.shape == aut.next.shape == (aut.num_states, Cn)
    assert np.isfinite(logp64).all()                                           # every probability > 0
    m = logp64.max(axis=1, keepdims=True)
    lse = (m + np.log(np.exp(logp64 - m).sum(axis=1, keepdims=True)))[:, 0]
    assert np.abs(lse).max() < 1e-6
    assert aut.next.min() >= 0 and aut.next.max() < aut.num_states and (aut.next[:, BLANK] == 0).all()
    assert aut.num_states == 1 + len(lm.kept) and (order > 1 or aut.num_states == 1)
    assert aut.start == (0 if order == 1 else aut.state_after([]))
    assert _exact(lm, aut, logp64, _prefixes(np.random.default_rng(order)))
    print(f"order {order}: S = {aut.num_states}")


def test_witten_bell_by_hand():
    # phrases "0 1" and "0 0": order 2, C = 4 (blank 3), smoothing 0.5
    lm = CharNGramLM.fit([[0, 1], [0, 0]], order=2, num_classes=4, smoothing=0.5)
    n = 6.0                                                  # events: 0 1 EOS 0 0 EOS
    p0 = (np.array([3, 1, 0, 2]) + 0.5) / (n + 0.5 * 4)
    # context (0): followed by 1, 0, EOS -> c = 3, t = 3
    want = (np.array([1, 1, 0, 1]) + 3 * p0) / (3 + 3)
    got = np.exp([lm.logprob([0], c) for c in range(4)])
    np.testing.assert_allclose(got, want, rtol=1e-15)
    # context (BOS): followed by 0 twice -> c = 2, t = 1
    np.testing.assert_allclose(np.exp([lm.logprob([], c) for c in range(4)]), (np.array([2, 0, 0, 0]) + p0) / 3, rtol=1e-15)
    # context (2) is unseen: the empty context
    np.testing.assert_allclose(np.exp([lm.logprob([2], c) for c in range(4)]), p0, rtol=1e-15)
    assert set(lm.kept) == {(BOS,), (0,), (1,)}


def test_dropping_the_backoff_in_next_is_caught():
    """The mutant: next goes to the empty context whenever the full context h + c is not kept (no longest-suffix search)."""
    lm = CharNGramLM.fit(_phrases(), order=4, num_classes=Cn)
    aut = lm.automaton()
    states = lm._states()
    index = {h: s for s, h in enumerate(states)}
    nxt = np.zeros_like(aut.next)
    for s, h in enumerate(states):
        for c in range(BLANK):
            g = (h + (c,))[-3:]
            nxt[s, c] = index.get(g, 0)
    assert (nxt != aut.next).any()
    mutant = LMAutomaton(aut.logp, nxt, aut.start)
    prefixes = _prefixes(np.random.default_rng(4))
    assert _exact(lm, aut, lm.logp_fp64(), prefixes)
    assert not _exact(lm, mutant, lm.logp_fp64(), prefixes)


def test_save_load_round_trip(tmp_path):
    lm = CharNGramLM.fit(_phrases(1), order=3, num_classes=Cn, smoothing=0.3)
    path = lm.save(str(tmp_path / "lm"))
    assert path.endswith(".npz")
    with np.load(path, allow_pickle=False) as z:             # data only: loads with pickling refused
        assert all(z[k].dtype != object for k in z.files)
    back = CharNGramLM.load(path)
    a, b = lm.automaton(), back.automaton()
    assert (back.order, back.blank, back.smoothing) == (3, BLANK, 0.3)
    assert np.array_equal(a.logp, b.logp) and np.array_equal(a.next, b.next) and a.start == b.start
    assert np.array_equal(lm.logp_fp64(), back.logp_fp64())


def test_max_states_prunes_the_longest_contexts_first():
    full = CharNGramLM.fit(_phrases(2), order=4, num_classes=Cn)
    S = full.automaton().num_states
    cap = S // 3
    lm = CharNGramLM.fit(_phrases(2), order=4, num_classes=Cn, max_states=cap)
    aut = lm.automaton()
    assert aut.num_states == cap < S
    assert np.abs(np.log(np.exp(lm.logp_fp64()).sum(axis=1))).max() < 1e-6
    assert _exact(lm, aut, lm.logp_fp64(), _prefixes(np.random.default_rng(7), 150))
    longest = max(len(h) for h in lm.kept)
    assert all(h in lm.kept for h in full.kept if len(h) < longest)           # nothing shorter went before the longest were gone
    again = CharNGramLM.fit(_phrases(2), order=4, num_classes=Cn, max_states=cap)
    assert sorted(again.kept) == sorted(lm.kept)
    assert CharNGramLM.fit(_phrases(2), order=4, num_classes=Cn, max_states=1).automaton().num_states == 1


def test_min_count_and_sampling():
    lm = CharNGramLM.fit(_phrases(3), order=3, num_classes=Cn, min_count=4)
    assert all(v.sum() >= 4 for v in lm.kept.values())
    assert _exact(lm, lm.automaton(), lm.logp_fp64(), _prefixes(np.random.default_rng(8), 100))
    g = np.random.default_rng(0)
    for _ in range(20):
        p = lm.sample(g, 12)
        assert len(p) <= 12 and all(0 <= c < Cn and c != BLANK for c in p)


def test_argument_errors():
    with pytest.raises(ValueError):
        CharNGramLM.fit([[1, 2]], order=0, num_classes=Cn)
    with pytest.raises(ValueError):
        CharNGramLM.fit([[1, 2]], order=9, num_classes=Cn)
    with pytest.raises(ValueError):
        CharNGramLM.fit([[1, BLANK, 2]], order=2, num_classes=Cn)
    with pytest.raises(ValueError):
        CharNGramLM.fit([[1, 2]], order=2, num_classes=Cn, smoothing=0.0)
    with pytest.raises(ValueError):
        CharNGramLM.fit(["ab"], order=2, num_classes=Cn)                       # strings need char_to_num
    with pytest.raises(ValueError):
        LMAutomaton(np.zeros((2, 4)), np.full((2, 4), 2), 0)                   # next outside [0, S)
    with pytest.raises(ValueError):
        LMAutomaton(np.zeros((2, 4)), np.zeros((2, 4)), 2)
    with pytest.raises(ValueError):
        LMAutomaton(np.zeros((2, 4)), np.zeros((2, 5)), 0)
    assert CharNGramLM.fit(["ab"], order=2, char_to_num={"a": 0, "b": 1}, num_classes=4).logprob([0], 1) > np.log(0.4)


# ------------------------------------------------------------------------------------------------ host search
def _bigram(seed=0):
    g = np.random.default_rng(seed)
    return CharBigramLM.fit([g.integers(0, BLANK, int(g.integers(3, 20))).tolist() for _ in range(200)], num_classes=Cn, smoothing=0.5)


def test_bigram_automaton_searches_exactly_as_the_table():
    g = np.random.default_rng(0)
    for case in range(40):                                   # the small shapes of test_ctc_beam.py
        T, Cc = int(g.integers(1, 7)), int(g.integers(2, 5))
        x = g.standard_normal((T, Cc)) * float(g.choice([0.5, 1.0, 3.0]))
        table = np.log(g.dirichlet(np.ones(Cc), Cc)).astype(np.float32)
        for W, nb in ((1, 1), (3, 2), (8, 8)):
            a = prefix_beam_search(x, W, nb, lm=table, alpha=0.7, beta=0.3, return_margin=True)
            b = prefix_beam_search(x, W, nb, lm=LMAutomaton.from_bigram(table), alpha=0.7, beta=0.3, return_margin=True)
            assert a[1] == b[1] and len(a[0]) == len(b[0])
            for (ia, sa), (ib, sb) in zip(a[0], b[0]):
                assert np.array_equal(ia, ib) and sa == sb
    lm = _bigram()
    x = 3.0 * g.standard_normal((48, Cn))
    for W in (1, 4, 16):
        a = prefix_beam_search(x, W, min(W, 2), lm=lm, alpha=0.4, beta=0.5)
        b = prefix_beam_search(x, W, min(W, 2), lm=LMAutomaton.from_bigram(lm), alpha=0.4, beta=0.5)
        assert [(i.tolist(), s) for i, s in a] == [(i.tolist(), s) for i, s in b]
    assert LMAutomaton.from_bigram(lm).start == BLANK


def test_order3_without_weight_is_the_search_without_lm():
    lm = CharNGramLM.fit(_phrases(5), order=3, num_classes=Cn)
    x = 2.0 * np.random.default_rng(6).standard_normal((40, Cn))
    a = prefix_beam_search(x, 1, 1, lm=lm, alpha=0.0, beta=0.2)
    b = prefix_beam_search(x, 1, 1, beta=0.2)
    assert [(i.tolist(), s) for i, s in a] == [(i.tolist(), s) for i, s in b]


def test_order3_score_is_the_sum_of_its_terms():
    """At a wide beam on a confident clip the top score is log p(path family) + alpha * (sum of logprob over the prefix + EOS) + beta * len."""
    lm = CharNGramLM.fit(_phrases(5), order=3, num_classes=Cn)
    seq = [3, 1, 4, 1, 5]
    x = np.zeros((2 * len(seq) + 1, Cn))
    x[:, BLANK] = 30.0
    for k, c in enumerate(seq):
        x[2 * k + 1, BLANK] = 0.0
        x[2 * k + 1, c] = 30.0
    (idx, score), = prefix_beam_search(x, 8, 1, lm=lm, alpha=0.6, beta=0.25)
    assert idx.tolist() == seq
    aut = lm.automaton()
    want = sum(float(aut.logp[aut.state_after(seq[:k]), c]) for k, c in enumerate(seq)) + float(aut.logp[aut.state_after(seq), BLANK])
    assert abs(score - (0.6 * want + 0.25 * len(seq))) < 1e-6              # the acoustic term is ~ -T * 59 e^-30


# ------------------------------------------------------------------------------------------------ dispatch, ABI
def test_entry_point_follows_the_type_of_lm():
    ngram = CharNGramLM.fit(_phrases(), order=3, num_classes=Cn)
    table = _bigram()
    for ragged in (False, True):
        assert entry_point(ngram, ragged) == "ishara_ctc_beam_decode_lm"
        assert entry_point(ngram.automaton(), ragged) == "ishara_ctc_beam_decode_lm"
        assert entry_point(LMAutomaton.from_bigram(table), ragged) == "ishara_ctc_beam_decode_lm"
        old = "ishara_ctc_beam_decode_ex" if ragged else "ishara_ctc_beam_decode"
        assert entry_point(None, ragged) == old
        assert entry_point(table, ragged) == old
        assert entry_point(np.asarray(table), ragged) == old
    assert as_automaton(ngram) is ngram.automaton() and as_automaton(table) is None and as_automaton(None) is None
    dev = DeviceAutomaton(ngram.automaton(), Cn, "cpu")
    assert entry_point(dev) == "ishara_ctc_beam_decode_lm" and dev.logp.dtype.is_floating_point and dev.S == ngram.automaton().num_states
    with pytest.raises(ValueError):
        DeviceAutomaton(ngram.automaton(), Cn - 1, "cpu")
    for name in ("ishara_ctc_beam_decode", "ishara_ctc_beam_decode_ex", "ishara_ctc_beam_decode_lm"):
        assert name in _lib.SIGNATURES


def test_lm_entry_point_refuses_before_any_launch(lib):
    """No GPU here: every refusal must come from the host-side checks (a launch would fail differently)."""
    import ctypes as C
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 255) // 256 * 256
    P = C.c_void_p

    def call(C_=Cn, W=4, nbest=1, T=8, B=1, blank=BLANK, S=3, start=0, logp=a, nxt=a + 1024, alpha=0.5, ws=a + 2048, fl=None):
        return lib.ishara_ctc_beam_decode_lm(P(a), B, T, C_, blank, W, nbest, P(logp) if logp else None, P(nxt) if nxt else None, S, start,
                                             C.c_float(alpha), C.c_float(0.0), P(ws), P(a), P(a), P(a), P(fl) if fl else None, None)
    for kw, word in ((dict(S=0), "S=0"), (dict(S=(1 << 22) + 1), "states"), (dict(start=3), "start_state"), (dict(start=-1), "start_state"),
                     (dict(logp=0), "null"), (dict(nxt=0), "null"), (dict(logp=a + 4), "16-byte"), (dict(nxt=a + 1032), "16-byte"),
                     (dict(C_=65), "C=65"), (dict(C_=1, blank=0), "C=1"), (dict(blank=60), "blank"), (dict(W=33), "beam_width"), (dict(W=0), "beam_width"),
                     (dict(nbest=5), "nbest"), (dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(B=-1), "B=-1"),
                     (dict(alpha=float("nan")), "finite"), (dict(ws=a + 2049), "4-byte"), (dict(fl=a + 3002), "frame_len")):
        assert call(**kw) != 0, kw
        assert word in lib.ishara_last_error().decode(), (kw, lib.ishara_last_error())
    assert lib.ishara_ctc_beam_decode_lm(None, 0, 8, Cn, BLANK, 4, 1, None, None, 1, 0, C.c_float(0.5), C.c_float(0), None, None, None, None, None, None) == 0
