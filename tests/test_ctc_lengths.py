"""CPU: per-clip frame counts in the CTC loss, decoders and aligner -- what can be checked without a GPU.  The Python surface exists and
validates on the host; the four `*_ex` entry points refuse before any HIP call (the mechanism of tests/test_ops_refusals.py: made-up
addresses and a NULL stream, a refused call dereferences nothing); the ragged host references are the per-clip loops; the fp64
restatement of tests/ctc_lengths_parity.py is the oracle on every loss case of tests/test_ctc_lengths_gpu.py, and with one of the mistakes
those cases are for switched on it is rejected by the GPU test's own inputs and bounds (2x a bound, or an integer mismatch)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_lengths_parity as R
import ctc_parity as P
import ishara_amd
from ishara_amd import _lib, ctc

N = None
EX = ["ishara_ctc_loss_ex", "ishara_greedy_decode_ex", "ishara_ctc_beam_decode_ex", "ishara_ctc_align_ex"]


def test_surface_is_exported():
    for n in ("ctc_loss", "ctc_greedy_decode", "ctc_beam_decode", "ctc_align"):
        assert callable(getattr(ishara_amd, n)), n
    assert set(EX) <= set(_lib.SIGNATURES)
    import inspect
    for m in ("ctc_loss", "decode_batch", "beam_decode", "align"):
        assert inspect.signature(getattr(ishara_amd.Model, m)).parameters["frame_lengths"].default is None
    for mod in (ishara_amd.ctc_beam, ishara_amd.ctc_align):
        assert inspect.signature(mod.launch).parameters["frame_len"].default is None


# ------------------------------------------------------------------ host validation of the wrapper
def _loss_args(**kw):
    a = dict(log_probs=torch.zeros(2, 9, 5), targets=torch.ones(2, 3, dtype=torch.long), input_lengths=[9, 4], target_lengths=[3, 0])
    a.update(kw)
    return a


@pytest.mark.parametrize("kw,word", [
    (dict(input_lengths=[9, 10]), "input_lengths"), (dict(input_lengths=[0, 9]), "input_lengths"), (dict(input_lengths=torch.tensor([9, -1])), "input_lengths"),
    (dict(input_lengths=[9]), "input_lengths"), (dict(input_lengths=[9.0, 4.0]), "input_lengths"),
    (dict(target_lengths=[4, 0]), "target_lengths"), (dict(target_lengths=[-1, 0]), "target_lengths"), (dict(target_lengths=np.array([[3, 0]])), "target_lengths"),
    (dict(log_probs=torch.zeros(2, 9, 65)), "C=65"), (dict(log_probs=torch.zeros(2, 9, 1)), "C=1"), (dict(log_probs=torch.zeros(9, 5)), "[B, T, C]"),
    (dict(targets=torch.ones(2, 256, dtype=torch.long)), "S=256"), (dict(targets=torch.ones(3, 3, dtype=torch.long)), "targets"),
    (dict(blank=5), "blank"), (dict(blank=-1), "blank"), (dict(reduction="batchmean"), "reduction"),
])
def test_ctc_loss_validates_on_the_host(kw, word):
    with pytest.raises(ValueError, match=word.replace("[", r"\[").replace("]", r"\]")):
        ishara_amd.ctc_loss(**_loss_args(**kw))


def test_valid_host_arguments_reach_the_device_check():
    """nothing is computed on the CPU: valid arguments with CPU logits are an error of their own, not a fallback"""
    with pytest.raises(_lib.IsharaError, match="GPU"):
        ishara_amd.ctc_loss(**_loss_args())
    for f, a in ((ishara_amd.ctc_greedy_decode, ()), (ishara_amd.ctc_beam_decode, ()), (ishara_amd.ctc_align, (np.zeros((2, 3), np.int64),))):
        with pytest.raises(ValueError, match="lengths"):
            f(torch.zeros(2, 9, 5), *a, lengths=[9, 10])
        with pytest.raises(_lib.IsharaError, match="GPU"):
            f(torch.zeros(2, 9, 5), *a, lengths=[9, 4])


def test_targets_are_packed_into_blank_padded_rows():
    y = ctc.pack_targets(torch.tensor([[3, 4, 5], [6, 7, 8]]), torch.tensor([2, 0]), 0, "cpu")
    assert y.dtype == torch.int64 and y.tolist() == [[3, 4, 0], [0, 0, 0]]
    assert ctc.pack_targets(torch.zeros(2, 0, dtype=torch.long), torch.tensor([0, 0]), 9, "cpu").tolist() == [[9], [9]]


# ------------------------------------------------------------------ refusals of the four entry points
P_ = {k: C.c_void_p(4096 * (i + 1)) for i, k in enumerate(("logits", "labels", "nll", "dlogits", "ws", "fl", "ss", "a", "b", "c", "d", "e"))}


def _call(lib, name, ptrs=None, flags=0, **kw):
    v = dict(B=2, T=16, C=60, L=8, blank=59, W=4, nbest=2)
    assert set(kw) <= set(v), kw
    v.update(kw)
    p = dict(P_)
    p.update(ptrs or {})
    f = C.c_float
    if name == "ishara_ctc_loss_ex":
        return lib.ishara_ctc_loss_ex(p["logits"], p["labels"], v["B"], v["T"], v["C"], v["L"], v["blank"], p["nll"], p["dlogits"], f(1.0), p["ws"], p["fl"], p["ss"], flags, N)
    if name == "ishara_greedy_decode_ex":
        return lib.ishara_greedy_decode_ex(p["logits"], v["B"], v["T"], v["C"], v["blank"], p["a"], p["b"], p["fl"], N)
    if name == "ishara_ctc_beam_decode_ex":
        return lib.ishara_ctc_beam_decode_ex(p["logits"], v["B"], v["T"], v["C"], v["blank"], v["W"], v["nbest"], N, f(0.0), f(0.0), p["ws"], p["a"], p["b"], p["c"], p["fl"], N)
    return lib.ishara_ctc_align_ex(p["logits"], p["labels"], v["B"], v["T"], v["C"], v["L"], v["blank"], p["ws"], p["a"], p["b"], p["c"], p["d"], p["e"], p["fl"], N)


def _refused(lib, rc, name, *words):
    msg = (lib.ishara_last_error() or b"").decode()
    assert rc != 0, f"{name}: accepted the call"
    assert msg.startswith(name + ":"), f"{name}: the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{name}: {msg!r} does not say {w!r}"


@pytest.mark.parametrize("name", EX)
def test_ex_refuses_what_its_sibling_refuses(lib, name):
    _refused(lib, _call(lib, name, B=-1), name, "B=-1")
    _refused(lib, _call(lib, name, T=0), name, "T=0")
    _refused(lib, _call(lib, name, blank=60), name, "blank 60")
    if name != "ishara_greedy_decode_ex":                                # the greedy decoder takes any class count
        _refused(lib, _call(lib, name, C=65, blank=0), name, "C=65")
    _refused(lib, _call(lib, name, ptrs=dict(logits=N)), name, "null")
    if name != "ishara_ctc_loss_ex":
        _refused(lib, _call(lib, name, T=4097), name, "4096")
    if name in ("ishara_ctc_loss_ex", "ishara_ctc_align_ex"):
        _refused(lib, _call(lib, name, L=256), name, "L=256", "1..255")
        _refused(lib, _call(lib, name, L=0), name, "L=0")
    if name == "ishara_ctc_loss_ex":
        _refused(lib, _call(lib, name, T=2 ** 31 - 1), name, "LDS")
        _refused(lib, _call(lib, name, ptrs=dict(ws=C.c_void_p(20484))), name, "ws", "8-byte")
    if name == "ishara_ctc_beam_decode_ex":
        _refused(lib, _call(lib, name, W=33), name, "beam_width 33")
        _refused(lib, _call(lib, name, nbest=5), name, "nbest 5")
    if name == "ishara_ctc_align_ex":
        _refused(lib, _call(lib, name, ptrs=dict(ws=C.c_void_p(20488))), name, "ws", "16-byte")


@pytest.mark.parametrize("name", EX)
def test_ex_refuses_a_misaligned_length_array(lib, name):
    for off in (1, 2, 3):
        _refused(lib, _call(lib, name, ptrs=dict(fl=C.c_void_p(24576 + off))), name, "frame_len", "4-byte")
    if name == "ishara_ctc_loss_ex":
        for off in (1, 2, 3):
            _refused(lib, _call(lib, name, ptrs=dict(ss=C.c_void_p(28672 + off))), name, "sample_scale", "4-byte")


def test_loss_ex_refuses_unknown_flag_bits(lib):
    for flags in (2, 3, 0x80000000, 0xFFFFFFFE):
        _refused(lib, _call(lib, "ishara_ctc_loss_ex", flags=flags), "ishara_ctc_loss_ex", "flag")


@pytest.mark.parametrize("name", EX)
def test_ex_of_an_empty_batch_is_a_no_op(lib, name):
    assert _call(lib, name, B=0, ptrs={k: N for k in P_}) == 0


# ------------------------------------------------------------------ the ragged host references are the per-clip loops
def test_ragged_host_references_are_the_per_clip_loops():
    from ishara_amd.ctc_align import viterbi_align
    from ishara_amd.ctc_beam import prefix_beam_search
    g = np.random.default_rng(5)
    x = g.standard_normal((3, 12, 6)).astype(np.float32)
    fl = [12, 5, 1]
    clips = ctc.ragged_clips(x, fl)
    assert [c.shape for c in clips] == [(12, 6), (5, 6), (1, 6)] and all(np.array_equal(c, x[b, :fl[b]]) for b, c in enumerate(clips))
    got = ctc.prefix_beam_search_ragged(x, fl, 4, nbest=2)
    for b in range(3):
        want = prefix_beam_search(x[b, :fl[b]], 4, nbest=2)
        assert len(got[b]) == len(want) and all(np.array_equal(p, q) and s == t for (p, s), (q, t) in zip(got[b], want))
    y = np.array([[1, 2, 5, 5], [3, 5, 5, 5], [2, 2, 5, 5]])
    fp, st, en, cf, sc = ctc.viterbi_align_ragged(x, y, fl, 5)
    for b in range(3):
        f, s, e, c, v = viterbi_align(x[b, :fl[b]], y[b], 5)
        assert np.array_equal(fp[b, :fl[b]], f) and (fp[b, fl[b]:] == -1).all()
        assert np.array_equal(st[b], s) and np.array_equal(en[b], e) and np.array_equal(cf[b], c) and sc[b] == v
    assert sc[2] == -1e30                                            # "2 2" needs three frames
    a = R.align_rows(x, y, fl, 5)
    assert all(np.array_equal(p, q) for p, q in zip(a, (fp, st, en, cf, sc)))


# ------------------------------------------------------------------ the restatement, clean and with the mistakes
LOSS_CASES = [R.tails(), R.seams(64), R.seams(255), R.contract(), R.scaled()]


def test_the_cases_are_what_they_claim():
    t = R.tails()
    assert t.B == 44 and R.feasible(t).all() and sorted(set(R.frame_len(t))) == list(P.B_TS)
    for L in (64, 255):
        s = R.seams(L)
        assert (2 * L + 1 + 63) // 64 == {64: 3, 255: 8}[L]
        tight, short = R.tight_index(s), R.short_index(s)
        assert len(tight) >= len([1 for n, _ in P.TIGHT if n <= L]) and len(short) >= len([1 for n, r in P.TIGHT if n <= L and n + len(r) > 1])
        assert R.feasible(s)[tight].all() and not R.feasible(s)[short].any()
        n, rep = P.lengths(s.base)
        assert (n + rep <= s.T).all()                                  # every label fits the buffer: only Tb can make a sample infeasible
        assert {129, 130, 272} <= set(R.frame_len(s))
    assert not R.feasible(R.scaled())[-1] and R.feasible(R.scaled())[:-1].all() and R.feasible(R.contract()).all()


@pytest.mark.parametrize("rc", LOSS_CASES, ids=lambda c: c.name)
@pytest.mark.parametrize("kind", ["normal", "nan"])
def test_unmutated_restatement_is_the_oracle(rc, kind):
    """the condition of the mutant test: with no mistake switched on the restatement passes every case, whatever the padding holds"""
    fl = R.frame_len(rc)
    nll, grad = R.restate(R.pad(R.logits(rc), fl, kind), R.labels(rc), rc.blank, fl)
    rn, rg = R.oracle(rc)
    ok = R.feasible(rc)
    assert np.allclose(nll[ok], rn[ok], rtol=1e-9, atol=1e-9) and np.allclose(grad, rg, rtol=1e-9, atol=1e-9)
    assert (nll[~ok] >= P.SENTINEL).all() and (grad[np.arange(rc.T)[None, :] >= fl[:, None]] == 0).all()
    obs, bad = R.compare(rc, nll, grad)
    assert not bad and max(obs.values()) < 1e-3, obs
    for b in R.tight_index(rc):
        v, g = R.closed_form(rc, b)
        assert abs(v - nll[b]) <= 1e-9 * max(1.0, abs(v)) and np.allclose(g, grad[b, :fl[b]], rtol=0, atol=1e-9)


def test_torch_ctc_loss_with_input_lengths_is_the_oracle_on_the_slice():
    """what the issue states about the second reference: F.ctc_loss with input_lengths equals the oracle on x[b, :Tb], and its gradient past
    the length is exactly 0"""
    rc = R.tails()
    x = torch.from_numpy(R.logits(rc).astype(np.float64)).requires_grad_(True)
    y, fl = R.labels(rc), R.frame_len(rc)
    tl = (y != rc.blank).sum(1)
    v = torch.nn.functional.ctc_loss(torch.log_softmax(x, -1).transpose(0, 1), torch.from_numpy(y.copy()), torch.from_numpy(fl.astype(np.int64)),
                                     torch.from_numpy(tl), blank=rc.blank, reduction="none")
    v.sum().backward()
    rn, rg = R.oracle(rc)
    assert np.allclose(v.detach().numpy(), rn, rtol=1e-12, atol=1e-10) and np.allclose(x.grad.numpy(), rg, rtol=0, atol=1e-10)
    assert (x.grad.numpy()[np.arange(rc.T)[None, :] >= fl[:, None]] == 0).all()


# mistake -> (case, padding, sample_scale): the GPU test runs exactly these inputs
MUTANT_CASES = {
    "beta_from_T": (R.tails(), "normal", None),
    "feasible_by_T": (R.seams(64), "normal", None),
    "pad_rows_softmax": (R.tails(), "normal", None),
    "next_length": (R.tails(), "normal", None),
    "tail_group": (R.tails(), "normal", None),
    "scale_nll": (R.scaled(), "normal", R.SCALES_ANY),
}
assert set(MUTANT_CASES) == set(R.MUTANTS)


@pytest.mark.parametrize("mut", sorted(R.MUTANTS))
def test_bounds_reject_the_mutant(mut):
    rc, kind, ss = MUTANT_CASES[mut]
    fl = R.frame_len(rc)
    nll, grad = R.restate(R.pad(R.logits(rc), fl, kind), R.labels(rc), rc.blank, fl, sample_scale=ss, mut=(mut,))
    obs, _ = R.compare(rc, nll.astype(np.float32), grad.astype(np.float32), sample_scale=ss)
    print(f"{mut} ({R.MUTANTS[mut]}): err / bound {obs}")
    assert max(obs.values()) >= 2.0, f"{mut}: no quantity exceeds 2x its bound: {obs}"


def test_decode_rows_reject_a_final_run_taken_at_the_buffers_end():
    for Cc in R.DECODE_CS:
        x, fl, blank = R.decode_batch(Cc)
        idx, ln = R.decode_rows(x, fl, blank)
        bad_idx, bad_ln = R.decode_rows(x, fl, blank, mut=("final_run_at_T",))
        short = fl < R.DECODE_T
        assert (ln[short] != bad_ln[short]).all() or not all(np.array_equal(a, b) for a, b in zip(idx[short], bad_idx[short]))
        for b in np.nonzero(short)[0][::2]:                            # form 0: the run that ends at Tb - 1 is what the mistake emits
            assert bad_ln[b] > ln[b] and bad_idx[b, ln[b]] == x[b, fl[b] - 1].argmax()
        for b in range(1, len(fl), 2):                                 # form 1: frame Tb - 2 is the last one kept
            if fl[b] >= 2:
                assert ln[b] >= 1 and idx[b, ln[b] - 1] == x[b, fl[b] - 2].argmax()


def test_align_rows_reject_frame_pos_left_unwritten():
    rc = R.align_case(64)
    fl = R.frame_len(rc)
    good = R.align_rows(R.logits(rc), R.labels(rc), fl, rc.blank)
    bad = R.align_rows(R.logits(rc), R.labels(rc), fl, rc.blank, mut=("frame_pos_unwritten",))
    assert (fl < rc.T).any() and not np.array_equal(good[0], bad[0]) and (good[0][np.arange(rc.T)[None, :] >= fl[:, None]] == -1).all()
    ok = R.feasible(rc)
    assert ok.any() and (~ok).any() and (good[4][~ok] == -1e30).all() and (good[4][ok] > -1e29).all()
