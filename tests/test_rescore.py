"""CPU: the host side of the second-pass n-best rescoring (ishara_amd/rescore.py) -- the fp64 forward algorithm against the oracle, torch and
the closed form; the properties of rescore_reference; the argument refusals of ishara_ctc_score_nbest and ishara_nbest_rescore through the C
ABI (refused before any HIP call: the device pointers here are made-up addresses); and the identity the GPU test relies on: where the beam
prunes nothing, the beam search's score is the exact CTC log-likelihood."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import ctc_parity as CP
import rescore_parity as P
from ishara_amd import mbr, rescore
from ishara_amd.ctc_beam import prefix_beam_search
from ishara_amd.ctc_lm import LMAutomaton
from oracle import ishara_oracle as O


# ------------------------------------------------------------------------------------------------ ctc_logp_reference
@pytest.mark.parametrize("blank", [7, 0, 3])
def test_forward_algorithm_equals_the_oracle_and_torch(blank):
    g = np.random.default_rng(50 + blank)
    Cn, T = 8, 21
    x = g.standard_normal((T, Cn)) * 2
    for n, rep in ((0, ()), (1, ()), (2, (1,)), (5, ()), (7, (2, 3)), (12, (5,)), (15, (1, 3, 5, 7, 9, 11))):
        h = P.make_hyp(g, n, rep, Cn, blank)
        got = rescore.ctc_logp_reference(x, h, blank)
        y = np.full((1, 16), blank, np.int64)
        y[0, :n] = h
        want = -float(O.ctc_nll(torch.from_numpy(y), torch.from_numpy(x[None]), blank)[0])
        assert abs(got - want) <= 1e-9, (n, rep, got, want)
        lp = torch.log_softmax(torch.from_numpy(x), -1)[:, None, :]
        tw = -float(torch.nn.functional.ctc_loss(lp, torch.tensor([h], dtype=torch.long).reshape(1, n), torch.tensor([T]), torch.tensor([n]), blank=blank,
                                                 reduction="none")[0])
        assert abs(got - tw) <= 1e-9, (n, rep, got, tw)


def test_one_alignment_is_the_closed_form_and_one_frame_less_is_impossible():
    g = np.random.default_rng(60)
    Cn, blank = 8, 7
    for n, rep in ((1, ()), (4, ()), (5, (2,)), (33, (32,)), (9, (1, 2, 3))):
        h = P.make_hyp(g, n, rep, Cn, blank)
        T = n + len(rep)
        x = g.standard_normal((T, Cn)) * 2
        path = CP.path_of(np.array(h, np.int64), n, blank, T)
        want = float(np.log(CP.softmax64(x))[np.arange(T), path].sum())
        assert abs(rescore.ctc_logp_reference(x, h, blank) - want) <= 1e-9 * max(1.0, abs(want))
        if T > 1:
            assert rescore.ctc_logp_reference(x[:-1], h, blank) == -np.inf
    x = g.standard_normal((6, Cn))
    assert abs(rescore.ctc_logp_reference(x, [], blank) - float(np.log(CP.softmax64(x))[:, blank].sum())) <= 1e-12      # the all-blank path


def test_forward_algorithm_refuses_bad_input():
    x = np.zeros((4, 5))
    for h in ([5], [-1], [4]):                               # outside [0, C), and the blank (C - 1)
        with pytest.raises(ValueError):
            rescore.ctc_logp_reference(x, h)
    with pytest.raises(ValueError):
        rescore.ctc_logp_reference(np.zeros((0, 5)), [])
    with pytest.raises(ValueError):
        rescore.ctc_logp_reference(x, [1], blank=5)


def test_beam_without_pruning_scores_exactly():
    """C 3, T 4: 2 symbols give at most 1 + 2 + 4 + 8 + 16 = 31 strings (15 of them have an alignment in 4 frames), so a beam of 32 prunes
    nothing and the beam's score of a hypothesis is the sum over all its alignments"""
    g = np.random.default_rng(70)
    for trial in range(4):
        x = g.standard_normal((4, 3)) * (2.0 if trial < 3 else 6.0)
        hyps = prefix_beam_search(x, 32, nbest=32, blank=2)
        strings = {tuple(h.tolist()) for h, _ in hyps}
        feasible = {s for k in range(5) for s in itertools.product((0, 1), repeat=k) if k + P.repeats_of(s) <= 4}
        assert strings == feasible
        for h, sc in hyps:
            ref = rescore.ctc_logp_reference(x, h, 2)
            assert abs(sc - ref) <= CP.NLL_ATOL + CP.NLL_RTOL * abs(ref), (h, sc, ref)
            assert abs(sc - ref) <= 1e-9


# ------------------------------------------------------------------------------------------------ rescore_reference
def test_dedupe_keeps_the_first_copy():
    hyps = [[1, 2], [3], [1, 2], None, [1], [1, 2, 0], [3]]
    order, score, live, post = rescore.rescore_reference(hyps, [[-5, -1, -0.5, -0.1, -3, -4, -0.2]])
    assert order.tolist() == [1, 4, 5, 0, 2, 3, 6]           # the copies in slots 2 and 6 die whatever their score; a prefix is no copy
    assert live.tolist() == [True, True, True, True, False, False, False]
    assert score[:4].tolist() == [-1, -3, -4, -5] and np.isneginf(score[4:]).all()


def test_ties_go_to_the_lower_slot_and_minus_inf_ranks_last_among_the_live():
    hyps = [[0], [1], [2], [3], None, [4]]
    order, score, live, post = rescore.rescore_reference(hyps, [[-2, -np.inf, -1, -2, 0, -1]])
    assert order.tolist() == [2, 5, 0, 3, 1, 4]
    assert live.tolist() == [True] * 5 + [False] and np.isneginf(score[4]) and post[4] == 0 and post[5] == 0
    assert abs(post.sum() - 1.0) < 1e-12 and post[0] == post[1] and post[2] == post[3]
    # -inf from one participating model of two is -inf
    order, score, live, post = rescore.rescore_reference([[0], [1]], [[-1, -2], [-np.inf, -3]])
    assert order.tolist() == [1, 0] and score.tolist() == [-5, -np.inf]
    # nothing finite: the posterior is all 0; a NaN never outranks a number
    order, score, live, post = rescore.rescore_reference([[0], [1], [2]], [[np.nan, -np.inf, -np.inf]])
    assert order.tolist() == [1, 2, 0] and (post == 0).all()


def test_a_model_without_a_positive_weight_is_not_read():
    hyps = [[0], [1], [2]]
    a = rescore.rescore_reference(hyps, [[-1, -2, -3], [np.nan] * 3, [np.nan] * 3], weights=[2.0, 0.0, -1.0])
    b = rescore.rescore_reference(hyps, [[-1, -2, -3]], weights=[2.0])
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and a[1].tolist() == [-2, -4, -6]


def test_the_score_is_float32_in_the_stated_order():
    f = np.float32
    lp = np.array([[-1.1, -2.3], [-0.7, -5.9]], f)
    w = np.array([0.3, 1.7], f)
    _, score, _, _ = rescore.rescore_reference([[0, 1], [2]], lp, weights=w, beta=0.37)
    for n, ln in ((0, 2), (1, 1)):
        s = f(f(0) + f(w[0] * lp[0, n]))
        s = f(s + f(w[1] * lp[1, n]))
        s = f(s + f(f(0.37) * f(ln)))
        assert s in score and score.dtype == np.float32


def test_lm_walk_is_the_ngram_logprob_summed():
    lm = P.ngram4()
    aut = lm.automaton()
    hyps = [[1, 2, 3, 4, 5], [], [6, 6, 6], [0, 1, 0, 1, 0, 1, 2]]
    order, score, live, _ = rescore.rescore_reference(hyps, [[0.0] * 4], weights=[0.0], lm=lm, alpha=1.0)
    for r, n in enumerate(order):
        h = hyps[n]
        want = sum(lm.logprob(h[:i], c) for i, c in enumerate(h)) + lm.logprob(h, lm.blank)
        assert abs(float(score[r]) - want) <= 1e-5 * max(1.0, abs(want)), (h, score[r], want)
    # the float32 walk, exactly
    h = hyps[3]
    l, s = np.float32(0), aut.start
    for c in h:
        l, s = np.float32(l + aut.logp[s, c]), aut.next[s, c]
    l = np.float32(l + aut.logp[s, lm.blank])
    assert l in score
    # a bigram table is the automaton whose state is the last character; the end-of-phrase term is there
    g = np.random.default_rng(3)
    table = P._log_softmax_rows(g, 8)
    _, sc, _, _ = rescore.rescore_reference([[1, 2]], [[0.0]], weights=[0.0], lm=table, alpha=1.0)
    assert abs(float(sc[0]) - float(table[7, 1] + table[1, 2] + table[2, 7])) <= 1e-6
    _, sc2, _, _ = rescore.rescore_reference([[1, 2]], [[0.0]], weights=[0.0], lm=LMAutomaton.from_bigram(table), alpha=1.0)
    assert sc2[0] == sc[0]


def test_posterior_sums_to_one_or_is_all_zero():
    for c in P.rescore_cases():
        lists = mbr.nbest_to_lists(c["hyp_idx"], c["hyp_len"])
        lp = P.host_logps(c)
        for b in range(c["B"]):
            order, score, live, post = rescore.rescore_reference(lists[b], lp[:, b], c["weights"], c["lm"], c["alpha"], c["beta"],
                                                                 1.0 if c["inv_temp"] is None else float(c["inv_temp"]), c["blank"])
            fin = live & np.isfinite(score)
            assert (post[~fin] == 0).all() and (abs(post.sum() - 1.0) < 1e-12 if fin.any() else (post == 0).all()), (c["name"], b)
            assert sorted(order.tolist()) == list(range(c["N"]))


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
A = 0x10000                                                  # a made-up, 256-byte aligned device address: a refused call never dereferences it


def _score(lib, logits=A, B=2, T=12, Cn=8, blank=7, idx=A, ln=A, N=4, Th=12, fl=None, logp=A, status=None):
    return lib.ishara_ctc_score_nbest(logits, B, T, Cn, blank, idx, ln, N, Th, fl, logp, status, None)


def _rescore(lib, idx=A, ln=A, B=2, N=4, Th=12, ptrs=(A,), M=None, w=A, lm_logp=None, lm_next=None, S=0, start=0, Cn=0, blank=0, alpha=0.0, beta=0.0,
             it=None, out_idx=A + 0x1000, out_len=A + 0x2000, out_score=A + 0x3000, post=None, perm=None):
    arr = (C.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
    return lib.ishara_nbest_rescore(idx, ln, B, N, Th, arr, len(ptrs) if M is None else M, w, lm_logp, lm_next, S, start, Cn, blank, C.c_float(alpha),
                                    C.c_float(beta), it, out_idx, out_len, out_score, post, perm, None)


@pytest.mark.parametrize("kw, word", [
    (dict(logits=None), "null"), (dict(idx=None), "null"), (dict(ln=None), "null"), (dict(logp=None), "null"),
    (dict(Cn=1), "C=1"), (dict(Cn=65, blank=0), "C=65"), (dict(T=0), "T=0"), (dict(T=4097), "T=4097"), (dict(Th=0), "Th=0"), (dict(Th=4097), "Th=4097"),
    (dict(N=0), "N=0"), (dict(N=65), "N=65"), (dict(blank=-1), "blank"), (dict(blank=8), "blank"), (dict(B=-1), "B=-1"),
    (dict(logits=A + 2), "aligned"), (dict(idx=A + 1), "aligned"), (dict(ln=A + 2), "aligned"), (dict(fl=A + 3), "aligned"), (dict(logp=A + 2), "aligned"),
    (dict(status=A + 1), "aligned"),
])
def test_score_refuses(lib, kw, word):
    assert _score(lib, **kw) == -1
    msg = lib.ishara_last_error().decode()
    assert msg.startswith("ishara_ctc_score_nbest:") and word in msg, msg


@pytest.mark.parametrize("kw, word", [
    (dict(idx=None), "null"), (dict(ln=None), "null"), (dict(ptrs=None, M=1), "null logp"), (dict(ptrs=(A, 0)), "logp[1]"), (dict(w=None), "weights"),
    (dict(out_idx=None), "null"), (dict(out_len=None), "null"), (dict(out_score=None), "null"),
    (dict(M=0), "M=0"), (dict(ptrs=(A,) * 9), "M=9"), (dict(N=0), "N=0"), (dict(N=65), "N=65"), (dict(Th=0), "Th=0"), (dict(Th=4097), "Th=4097"), (dict(B=-1), "B=-1"),
    (dict(alpha=float("nan")), "finite"), (dict(beta=float("inf")), "finite"),
    (dict(lm_logp=A, lm_next=A, S=0, Cn=8, blank=7), "S=0"), (dict(lm_logp=A, lm_next=A, S=4, start=4, Cn=8, blank=7), "start_state"),
    (dict(lm_logp=A, lm_next=A, S=4, Cn=65, blank=7), "C=65"), (dict(lm_logp=A, lm_next=A, S=4, Cn=8, blank=8), "blank"),
    (dict(lm_logp=A, lm_next=None, S=4, Cn=8, blank=7), "together"), (dict(lm_logp=A + 4, lm_next=A, S=4, Cn=8, blank=7), "16-byte"),
    (dict(idx=A + 2), "aligned"), (dict(ptrs=(A, A + 1)), "aligned"), (dict(w=A + 2), "aligned"), (dict(it=A + 1), "aligned"), (dict(post=A + 0x4002), "aligned"),
    (dict(perm=A + 0x5001), "aligned"),
    (dict(out_idx=A), "overlaps"), (dict(out_len=A + 4), "overlaps"), (dict(out_score=A), "overlaps"), (dict(post=A + 8), "overlaps"), (dict(perm=A), "overlaps"),
])
def test_rescore_refuses(lib, kw, word):
    assert _rescore(lib, **kw) == -1
    msg = lib.ishara_last_error().decode()
    assert msg.startswith("ishara_nbest_rescore:") and word in msg, msg


def test_an_empty_batch_is_accepted_without_buffers(lib):
    assert _score(lib, logits=None, idx=None, ln=None, logp=None, B=0) == 0
    assert _rescore(lib, idx=None, ln=None, ptrs=None, M=1, w=None, out_idx=None, out_len=None, out_score=None, B=0) == 0
    assert lib.ishara_debug_set_score_group(0) == 0


def test_the_wrappers_refuse_host_tensors_and_bad_shapes():
    idx, ln = torch.zeros((2, 3, 5), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="GPU"):
        rescore.ctc_score_nbest(torch.zeros((2, 4, 8)), idx, ln)
    with pytest.raises(ValueError, match="GPU"):
        rescore.rescore_nbest(idx, ln, torch.zeros((2, 3)))
    with pytest.raises(ValueError):
        rescore.rescore_reference([[0]], [[0.0, 1.0]])
    with pytest.raises(ValueError):
        rescore.rescore_reference([[0]], [[0.0]], weights=[1.0, 2.0])
    with pytest.raises(ValueError):
        rescore.rescore_models([], None, (idx, ln))
