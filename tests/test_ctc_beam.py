"""CPU: the host reference of the CTC prefix beam search (ishara_amd/ctc_beam.py) against an exhaustive sum over alignments and against
torch's CTC loss, the character-bigram LM and its fusion, and the ABI of ishara_ctc_beam_decode."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import torch

from ishara_amd import _lib
from ishara_amd.ctc_beam import CharBigramLM, log_softmax, prefix_beam_search


def _collapse(path, blank):
    out, prev = [], None
    for s in path:
        if s != prev and s != blank:
            out.append(s)
        prev = s
    return tuple(out)


def _exhaustive(logits, blank):
    """Every labeling's log-probability: the sum over all C^T alignments, in fp64."""
    lp = log_softmax(logits)
    T, Cc = lp.shape
    tot = {}
    for path in itertools.product(range(Cc), repeat=T):
        v = float(sum(lp[t, s] for t, s in enumerate(path)))
        k = _collapse(path, blank)
        tot[k] = np.logaddexp(tot[k], v) if k in tot else v
    return tot


def test_reference_equals_exhaustive_search():
    g = np.random.default_rng(0)
    checked = total = 0
    for case in range(120):
        T, Cc = int(g.integers(1, 7)), int(g.integers(2, 5))
        x = g.standard_normal((T, Cc)) * float(g.choice([0.5, 1.0, 3.0]))
        blank = Cc - 1
        tot = _exhaustive(x, blank)
        ranked = sorted(tot.items(), key=lambda kv: -kv[1])
        hyps = prefix_beam_search(x, 10 ** 4, nbest=1)
        (idx, score), = hyps
        # nothing is pruned at W = 10^4: the top-1 log-probability is exact, the labeling wherever the answer is not a near-tie
        assert abs(score - ranked[0][1]) < 1e-9, (case, score, ranked[0][1])
        assert abs(score - tot[tuple(idx.tolist())]) < 1e-9
        total += 1
        if len(ranked) == 1 or ranked[0][1] - ranked[1][1] > 1e-6:
            checked += 1
            assert tuple(idx.tolist()) == ranked[0][0], case
    assert checked >= 0.9 * total, (checked, total)


def test_reference_nbest_lists_every_labeling_unpruned():
    g = np.random.default_rng(1)
    x = g.standard_normal((4, 3))
    tot = _exhaustive(x, 2)
    hyps = prefix_beam_search(x, 10 ** 4, nbest=len(tot) + 3)
    assert len(hyps) == len(tot)                              # no more hypotheses than labelings
    assert len({tuple(i.tolist()) for i, _ in hyps}) == len(hyps)
    for i, s in hyps:
        assert abs(s - tot[tuple(i.tolist())]) < 1e-9
    sc = [s for _, s in hyps]
    assert all(a >= b for a, b in zip(sc, sc[1:]))


@pytest.mark.parametrize("W", [1, 3, 8])
def test_scores_bounded_by_torch_ctc_loss(W):
    g = np.random.default_rng(10 + W)
    for case in range(12):
        T, Cc = int(g.integers(3, 30)), int(g.integers(3, 12))
        x = g.standard_normal((T, Cc)) * 2.0
        hyps = prefix_beam_search(x, W, nbest=W)
        lp = torch.from_numpy(log_softmax(x)).unsqueeze(1)          # [T, 1, C] fp64
        for idx, score in hyps:
            tgt = torch.from_numpy(idx.astype(np.int64)).unsqueeze(0)
            nll = torch.nn.functional.ctc_loss(lp, tgt, torch.tensor([T]), torch.tensor([idx.size]), blank=Cc - 1, reduction="none",
                                               zero_infinity=False)
            assert score <= -float(nll[0]) + 1e-6, (case, idx, score, -float(nll[0]))
    # unpruned: equal
    x = g.standard_normal((5, 3))
    for idx, score in prefix_beam_search(x, 10 ** 4, nbest=5):
        lp = torch.from_numpy(log_softmax(x)).unsqueeze(1)
        nll = torch.nn.functional.ctc_loss(lp, torch.from_numpy(idx).unsqueeze(0), torch.tensor([5]), torch.tensor([idx.size]), blank=2,
                                           reduction="none")
        assert abs(score + float(nll[0])) < 1e-9


def test_last_frame_is_used_unlike_greedy():
    # one confident non-blank frame at the very end: greedy (c8:7-9) never emits the final run, the beam search does
    x = np.full((3, 4), -10.0)
    x[:2, 3] = 10.0
    x[2, 1] = 10.0
    (idx, _), = prefix_beam_search(x, 4)
    assert idx.tolist() == [1]


def test_uniform_logits_follow_the_tie_order():
    # every candidate of frame 0 ties: the same-prefix candidate first, then extensions by class index
    hyps = prefix_beam_search(np.zeros((1, 5)), 3, nbest=3)
    assert [h[0].tolist() for h in hyps] == [[], [0], [1]]
    hyps = prefix_beam_search(np.zeros((1, 5)), 3, nbest=3, return_margin=True)
    assert hyps[1] == 0.0                                     # exact ties: no margin


def test_char_bigram_lm_fit_rows_normalised(tmp_path):
    phrases = ["abc", "abd", "a", "+1-555"]
    chars = sorted(set("".join(phrases)))
    c2n = {c: i for i, c in enumerate(chars)}
    lm = CharBigramLM.fit(phrases, c2n, num_classes=12, smoothing=0.5)
    t = np.asarray(lm)
    assert t.shape == (12, 12) and t.dtype == np.float32
    np.testing.assert_allclose(np.exp(t.astype(np.float64)).sum(axis=1), 1.0, atol=1e-6)
    assert t[11, c2n["a"]] > t[11, c2n["b"]]                  # BOS -> 'a' is the most frequent start
    assert t[c2n["a"], c2n["b"]] > t[c2n["a"], c2n["c"]]
    assert t[c2n["c"], 11] > t[c2n["c"], c2n["a"]]            # 'c' ends a phrase
    p = lm.save(str(tmp_path / "lm"))
    np.testing.assert_array_equal(np.asarray(CharBigramLM.load(p)), t)
    with pytest.raises(ValueError):
        CharBigramLM.fit([[0, 11]], num_classes=12)           # the blank is not a character
    idx = CharBigramLM.fit([[0, 1, 2]], num_classes=5)
    assert np.asarray(idx).shape == (5, 5)


def test_lm_fusion_selects_the_preferred_character():
    # frames: blank, (a | b equally likely), blank.  Acoustically a tie; the LM prefers 'b' after BOS.
    Cc, blank, a, b = 4, 3, 0, 1
    x = np.full((3, Cc), -20.0)
    x[0, blank] = x[2, blank] = 0.0
    x[1, a] = x[1, b] = 0.0
    lm = CharBigramLM.fit([[b]] * 9 + [[a]], num_classes=Cc)
    (i0, s0), = prefix_beam_search(x, 4)
    assert i0.tolist() == [a]                                  # no LM: the tie goes to the lower class index
    (i1, s1), = prefix_beam_search(x, 4, lm=lm, alpha=0.5)
    assert i1.tolist() == [b]
    t = np.asarray(lm).astype(np.float64)
    assert abs(s1 - (s0 + 0.5 * (t[blank, b] + t[b, blank]))) < 1e-9
    (i2, _), = prefix_beam_search(x, 4, lm=lm, alpha=0.0)     # alpha = 0: the LM is off
    assert i2.tolist() == [a]
    (i3, s3), = prefix_beam_search(x, 4, beta=2.0)            # the length bonus is per emitted character
    assert abs(s3 - (s0 + 2.0)) < 1e-9


def test_reference_rejects_bad_arguments():
    x = np.zeros((3, 4))
    with pytest.raises(ValueError):
        prefix_beam_search(x, 2, nbest=3)
    with pytest.raises(ValueError):
        prefix_beam_search(x, 2, lm=np.zeros((3, 3)), alpha=1.0)
    with pytest.raises(ValueError):
        prefix_beam_search(x[0], 2)


def test_beam_symbols_in_the_abi(lib):
    for name in ("ishara_ctc_beam_workspace_bytes", "ishara_ctc_beam_decode"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ishara_ctc_beam_workspace_bytes(4, 384, 60, 16) == 4 * (1 + 384 * 16) * 4
    assert lib.ishara_ctc_beam_workspace_bytes(4, 384, 60, 33) < 0
    # limits are checked before anything touches the device: every call below fails with a message, B = 0 included
    bad = [(60, 59, 0, 1), (60, 59, 33, 1), (60, 59, 4, 5), (65, 64, 4, 1), (1, 0, 1, 1), (60, 60, 4, 1)]
    for Cc, blank, W, nb in bad:
        rc = lib.ishara_ctc_beam_decode(None, 0, 16, Cc, blank, W, nb, None, C.c_float(0), C.c_float(0), None, None, None, None, None)
        assert rc != 0
        assert lib.ishara_last_error()
    rc = lib.ishara_ctc_beam_decode(None, 0, 5000, 60, 59, 4, 1, None, C.c_float(0), C.c_float(0), None, None, None, None, None)
    assert rc != 0
    rc = lib.ishara_ctc_beam_decode(None, 0, 16, 60, 59, 4, 1, None, C.c_float(math.nan), C.c_float(0), None, None, None, None, None)
    assert rc != 0
    # B = 0 with valid limits is a no-op
    assert lib.ishara_ctc_beam_decode(None, 0, 16, 60, 59, 4, 1, None, C.c_float(0), C.c_float(0), None, None, None, None, None) == 0
