"""Per-sample frame counts in the CTC loss, the greedy decoder, the beam search and the aligner (the `*_ex` entry points) on the GPU.

Primary criterion: every output of sample b is bit-equal to the existing fixed-T entry point launched on that sample alone at T = Tb on
logits[b, :Tb] -- the route tests/test_ctc_gpu.py, test_ctc_beam_gpu.py and test_ctc_align_gpu.py pin to the fp64 oracle and the host
references.  No tolerance, no sample left out.  Second: nll and dlogits against the fp64 oracle on the slice, within ctc_parity's bounds;
the decoders and the aligner against decode_phrase / viterbi_align of the slice, exactly.  Cases and references: tests/ctc_lengths_parity.py.

Every buffer of every launch lies between two 4 KiB guard regions that must come back unchanged; float outputs are pre-filled with 0xFF
bytes (NaN) and integer outputs with 0x7F bytes (0xFF would read as the -1 padding the kernels have to write themselves)."""
import ctypes as C

import numpy as np
import pytest
import torch

import ctc_lengths_parity as R
import ctc_parity as P
import ishara_amd
from ishara_amd import _lib

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 4096, 0xA5
F = C.c_float


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guarded:
    """nbytes of device memory between two guard regions"""

    def __init__(self, nbytes, fill=0xFF):
        self.n = int(nbytes)
        self.buf = torch.full((2 * GUARD + self.n,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
        self.inner = self.buf[GUARD:GUARD + self.n]
        self.inner.fill_(fill)

    @classmethod
    def of(cls, a):
        t = torch.from_numpy(np.array(a, order="C"))
        g = cls(t.numel() * t.element_size())
        g.inner.copy_(t.view(-1).view(torch.uint8))
        return g

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + GUARD)

    def get(self, dtype, *shape):
        return self.inner.view(dtype).view(*shape).cpu().numpy()

    def check(self, name):
        lo, hi = self.buf[:GUARD].cpu().numpy(), self.buf[GUARD + self.n:].cpu().numpy()
        assert (lo == GUARD_BYTE).all() and (hi == GUARD_BYTE).all(), f"{name}: bytes outside the buffer were written"


def _finish(bufs):
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(np.asarray(a, np.float32)), bits(np.asarray(b, np.float32)))


# ------------------------------------------------------------------ the launches
def loss_ex(lib, x, y, blank, fl="null", ss=None, flags=0, gs=1.0, grad=True, ws_fill=0xFF):
    """one ishara_ctc_loss_ex launch -> (nll [B], grad [B, T, C] or None); fl = "null": frame_len NULL"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.int64)
    B, T, Cc = x.shape
    L = y.shape[1]
    bufs = dict(logits=Guarded.of(x), labels=Guarded.of(y), nll=Guarded(4 * B), ws=Guarded(int(lib.ishara_ctc_workspace_bytes(B, T, L)), ws_fill))
    if grad:
        bufs["dlogits"] = Guarded(4 * B * T * Cc)
    if not isinstance(fl, str):
        bufs["frame_len"] = Guarded.of(np.asarray(fl, np.int32))
    if ss is not None:
        bufs["sample_scale"] = Guarded.of(np.asarray(ss, np.float32))
    p = {k: v.ptr() for k, v in bufs.items()}
    _lib.check(lib.ishara_ctc_loss_ex(p["logits"], p["labels"], B, T, Cc, L, blank, p["nll"], p.get("dlogits"), F(gs), p["ws"], p.get("frame_len"),
                                      p.get("sample_scale"), flags, stream()), "ishara_ctc_loss_ex")
    _finish(bufs)
    return bufs["nll"].get(torch.float32, B), bufs["dlogits"].get(torch.float32, B, T, Cc) if grad else None


def loss_fixed(lib, x, y, blank, gs=1.0, grad=True):
    """the existing entry point"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.int64)
    B, T, Cc = x.shape
    L = y.shape[1]
    bufs = dict(logits=Guarded.of(x), labels=Guarded.of(y), nll=Guarded(4 * B), ws=Guarded(int(lib.ishara_ctc_workspace_bytes(B, T, L))))
    if grad:
        bufs["dlogits"] = Guarded(4 * B * T * Cc)
    p = {k: v.ptr() for k, v in bufs.items()}
    _lib.check(lib.ishara_ctc_loss(p["logits"], p["labels"], B, T, Cc, L, blank, p["nll"], p.get("dlogits"), F(gs), p["ws"], stream()), "ishara_ctc_loss")
    _finish(bufs)
    return bufs["nll"].get(torch.float32, B), bufs["dlogits"].get(torch.float32, B, T, Cc) if grad else None


def loss_solo(lib, x, y, blank, fl, gs=1.0):
    """the primary reference: sample by sample, the existing entry point at T = Tb on x[b, :Tb] -> (nll [B], [grad [Tb, C]])"""
    nll, grads = np.zeros(len(fl), np.float32), []
    for b, tb in enumerate(fl):
        n, g = loss_fixed(lib, x[b:b + 1, :tb], y[b:b + 1], blank, gs)
        nll[b] = n[0]
        grads.append(g[0])
    return nll, grads


def check_against_solo(name, nll, grad, solo, fl):
    snll, sgrad = solo
    for b, tb in enumerate(fl):
        assert bits(nll)[b] == bits(snll)[b], f"{name}: sample {b} (Tb = {tb}): nll {nll[b]!r} is not the solo launch's {snll[b]!r}"
        assert np.array_equal(bits(grad[b, :tb]), bits(sgrad[b])), f"{name}: sample {b} (Tb = {tb}): dlogits differ from the solo launch"
        assert not bits(grad[b, tb:]).any(), f"{name}: sample {b} (Tb = {tb}): dlogits past the sample's end is not +0"


def check_against_oracle(rc, nll, grad, **kw):
    obs, bad = R.compare(rc, nll, grad, **kw)
    print(rc.name, {k: f"{v:.3g}" for k, v in obs.items()})
    assert not bad, bad


# ------------------------------------------------------------------ loss: group tails, register seams
def _ragged_loss(lib, rc):
    x, y, fl = R.logits(rc), R.labels(rc), R.frame_len(rc)
    out = {kind: loss_ex(lib, R.pad(x, fl, kind), y, rc.blank, fl) for kind in R.PADS}
    nll, grad = out["normal"]
    for kind in ("nan", "inf"):
        assert same(out[kind][0], nll) and same(out[kind][1], grad), f"{rc.name}: outputs depend on rows past the samples' ends ({kind})"
    check_against_solo(rc.name, nll, grad, loss_solo(lib, x, y, rc.blank, fl), fl)
    check_against_oracle(rc, nll, grad)
    return nll, grad


def test_loss_group_tails(lib):
    """buffer T = 33: one sample per Tb in 1 .. 33 around the 8-frame groups and the 16-frame gradient stride, four label lengths each;
    the rows past each sample's end hold N(0, 2^2), then NaN, then +inf"""
    rc = R.tails()
    nll, grad = _ragged_loss(lib, rc)
    x, y, fl = R.logits(rc), R.labels(rc), R.frame_len(rc)
    for fill in (0xFF, 0x00):                                            # the workspace needs no initialisation
        n2, g2 = loss_ex(lib, R.pad(x, fl, "nan"), y, rc.blank, fl, ws_fill=fill)
        assert same(n2, nll) and same(g2, grad), "the outputs depend on what the workspace held"
    only, _ = loss_ex(lib, R.pad(x, fl, "nan"), y, rc.blank, fl, grad=False)
    assert same(only, nll), "nll without dlogits differs"


@pytest.mark.parametrize("L", [64, 255])
def test_loss_register_seams(lib, L):
    """buffer T = 272, NS = 3 and 8: the single-alignment samples at Tb = len + repeats (also against the closed form), one frame short
    (infeasible by Tb although the buffer would hold the label) and at Tb = T; the seam samples at Tb = 129, 130, T"""
    rc = R.seams(L)
    nll, grad = _ragged_loss(lib, rc)
    fl = R.frame_len(rc)
    for b in R.short_index(rc):
        assert nll[b] >= P.SENTINEL and np.isfinite(grad[b]).all(), f"sample {b}: a label that does not fit Tb = {fl[b]} was aligned"
    for b in R.tight_index(rc):
        v, g = R.closed_form(rc, b)
        assert abs(nll[b] - v) <= P.NLL_ATOL + P.NLL_RTOL * abs(v)
        assert (np.abs(grad[b, :fl[b]] - g) <= P.GRAD_ATOL + P.GRAD_RTOL * np.abs(g)).all()


# ------------------------------------------------------------------ loss: the contract
@pytest.mark.parametrize("case", [P.case_a(32), P.case_a(255), P.case_b(8, 9), P.case_b(64, 9)], ids=lambda c: c.name)
def test_loss_without_lengths_is_the_fixed_entry_point(lib, case):
    x, y = P.logits(case), P.labels(case)
    want = loss_fixed(lib, x, y, case.blank)
    for fl in ("null", np.full(case.B, case.T, np.int32)):
        got = loss_ex(lib, x, y, case.blank, fl)
        assert same(got[0], want[0]) and same(got[1], want[1])
    assert same(loss_ex(lib, x, y, case.blank, grad=False)[0], want[0])


def test_loss_out_of_range_lengths(lib):
    """frame_len 0, -3, T + 1 and 2^31 - 1 between feasible samples: the sentinel, an all-zero gradient, and neighbours bit-identical to a
    launch in which that sample has a valid length and an empty label (the logits lie inside a larger allocation: the guards)"""
    rc = R.contract()
    x, y, fl = R.logits(rc), R.labels(rc).copy(), R.frame_len(rc).astype(np.int64)
    odd = [1, 3, 5, 7]
    fl_bad = fl.copy()
    fl_bad[odd] = R.BAD_LENGTHS
    nll, grad = loss_ex(lib, x, y, rc.blank, fl_bad.astype(np.int32), gs=0.5)
    y2, fl2 = y.copy(), fl.copy()
    y2[odd], fl2[odd] = rc.blank, rc.T
    n2, g2 = loss_ex(lib, x, y2, rc.blank, fl2.astype(np.int32), gs=0.5)
    for b in range(rc.B):
        if b in odd:
            assert nll[b] >= P.SENTINEL and not bits(grad[b]).any(), f"sample {b} (frame_len {fl_bad[b]})"
        else:
            assert bits(nll)[b] == bits(n2)[b] and np.array_equal(bits(grad[b]), bits(g2[b])), f"sample {b}: a neighbour's length changed its outputs"
    even = [b for b in range(rc.B) if b not in odd]
    check_against_oracle(rc, nll, grad, grad_scale=0.5, only=even)


def test_loss_sample_scale_and_zero_infeasible(lib):
    rc = R.scaled()
    x, y, fl = R.logits(rc), R.labels(rc), R.frame_len(rc)
    xn = R.pad(x, fl, "nan")
    nll, grad = loss_ex(lib, xn, y, rc.blank, fl)
    assert nll[-1] >= P.SENTINEL and R.feasible(rc)[:-1].all()
    check_against_oracle(rc, nll, grad)
    n2, g2 = loss_ex(lib, xn, y, rc.blank, fl, ss=R.SCALES_POW2)
    assert same(n2, nll), "sample_scale reached nll"
    assert same(g2, R.SCALES_POW2[:, None, None] * grad), "a power-of-two sample_scale is not an exact factor of the gradient"
    n3, g3 = loss_ex(lib, xn, y, rc.blank, fl, ss=R.SCALES_ANY, gs=0.5)
    assert same(n3, nll)
    check_against_oracle(rc, n3, g3, grad_scale=0.5, sample_scale=R.SCALES_ANY)
    ref = R.restate(xn, y, rc.blank, fl)                                 # the restatement states the same contract
    check_against_oracle(rc, n3, g3, grad_scale=0.5, sample_scale=R.SCALES_ANY, ref=ref)
    n4, g4 = loss_ex(lib, xn, y, rc.blank, fl, flags=1)
    assert same(n4, nll) and not bits(g4[-1]).any(), "ISHARA_CTC_ZERO_INFEASIBLE: nll stays, the infeasible sample's gradient is +0"
    assert same(g4[:-1], grad[:-1])
    check_against_oracle(rc, n4, g4, zero_inf=True)


# ------------------------------------------------------------------ greedy
@pytest.mark.parametrize("Cc", R.DECODE_CS)
def test_greedy_decode_with_lengths(lib, Cc):
    """buffer T = 513, Tb around the 256-frame rounds: the whole out_idx row and out_len equal decode_phrase(x[b, :Tb]) padded with -1 to T"""
    x, fl, blank = R.decode_batch(Cc)
    B, T, _ = x.shape
    want_idx, want_len = R.decode_rows(x, fl, blank)
    for kind in ("normal", "nan"):
        bufs = dict(logits=Guarded.of(R.pad(x, fl, kind)), out_idx=Guarded(4 * B * T, 0x7F), out_len=Guarded(4 * B, 0x7F), frame_len=Guarded.of(fl))
        p = {k: v.ptr() for k, v in bufs.items()}
        _lib.check(lib.ishara_greedy_decode_ex(p["logits"], B, T, Cc, blank, p["out_idx"], p["out_len"], p["frame_len"], stream()), "ishara_greedy_decode_ex")
        _finish(bufs)
        idx, ln = bufs["out_idx"].get(torch.int32, B, T), bufs["out_len"].get(torch.int32, B)
        for b in range(B):
            assert ln[b] == want_len[b] and np.array_equal(idx[b], want_idx[b]), f"C={Cc} sample {b} (Tb = {fl[b]}, padding {kind}): decode differs"
    # NULL and all-T lengths: the existing entry point; an out-of-range length: nothing decoded
    ref = dict(logits=Guarded.of(x), out_idx=Guarded(4 * B * T, 0x7F), out_len=Guarded(4 * B, 0x7F))
    _lib.check(lib.ishara_greedy_decode(ref["logits"].ptr(), B, T, Cc, blank, ref["out_idx"].ptr(), ref["out_len"].ptr(), stream()), "ishara_greedy_decode")
    _finish(ref)
    fl_bad = np.full(B, T, np.int32)
    fl_bad[[1, 3, 5, 7]] = R.BAD_LENGTHS[:2] + (T + 1, 2 ** 31 - 1)
    for lens in (None, np.full(B, T, np.int32), fl_bad):
        bufs = dict(logits=Guarded.of(x), out_idx=Guarded(4 * B * T, 0x7F), out_len=Guarded(4 * B, 0x7F))
        if lens is not None:
            bufs["frame_len"] = Guarded.of(lens)
        p = {k: v.ptr() for k, v in bufs.items()}
        _lib.check(lib.ishara_greedy_decode_ex(p["logits"], B, T, Cc, blank, p["out_idx"], p["out_len"], p.get("frame_len"), stream()), "ishara_greedy_decode_ex")
        _finish(bufs)
        idx, ln = bufs["out_idx"].get(torch.int32, B, T), bufs["out_len"].get(torch.int32, B)
        for b in range(B):
            if lens is fl_bad and b in (1, 3, 5, 7):
                assert ln[b] == 0 and (idx[b] == -1).all()
            else:
                assert ln[b] == ref["out_len"].get(torch.int32, B)[b] and np.array_equal(idx[b], ref["out_idx"].get(torch.int32, B, T)[b])


# ------------------------------------------------------------------ beam
def _beam(lib, x, W, nbest, lm, alpha, beta, fl="fixed"):
    x = np.asarray(x, np.float32)
    B, T, Cc = x.shape
    bufs = dict(logits=Guarded.of(x), ws=Guarded(max(int(lib.ishara_ctc_beam_workspace_bytes(B, T, Cc, W)), 4)), out_idx=Guarded(4 * B * nbest * T, 0x7F),
                out_len=Guarded(4 * B * nbest, 0x7F), out_score=Guarded(4 * B * nbest))
    if lm is not None:
        bufs["lm"] = Guarded.of(lm)
    if not isinstance(fl, str):
        bufs["frame_len"] = Guarded.of(np.asarray(fl, np.int32))
    p = {k: v.ptr() for k, v in bufs.items()}
    a = (p["logits"], B, T, Cc, Cc - 1, W, nbest, p.get("lm"), F(alpha), F(beta), p["ws"], p["out_idx"], p["out_len"], p["out_score"])
    if isinstance(fl, str) and fl == "fixed":
        _lib.check(lib.ishara_ctc_beam_decode(*a, stream()), "ishara_ctc_beam_decode")
    else:
        _lib.check(lib.ishara_ctc_beam_decode_ex(*a, p.get("frame_len"), stream()), "ishara_ctc_beam_decode_ex")
    _finish(bufs)
    return bufs["out_idx"].get(torch.int32, B, nbest, T), bufs["out_len"].get(torch.int32, B, nbest), bufs["out_score"].get(torch.float32, B, nbest)


@pytest.mark.parametrize("use_lm", [False, True], ids=["nolm", "lm"])
@pytest.mark.parametrize("W", R.BEAM_WS)
def test_beam_decode_with_lengths(lib, W, use_lm):
    """buffer T = 40, Tb around the 16-frame chunk (and the 4-frame chunk of a one-wave launch), NaN past each clip's end: hypotheses,
    lengths and scores bit-equal to the solo launches -- the same arithmetic on both sides, so no near-tie allowance"""
    x, fl, lm = R.beam_batch()
    B, T, _ = x.shape
    nbest = min(W, 2)
    kw = dict(lm=lm if use_lm else None, alpha=0.7 if use_lm else 0.0, beta=0.3 if use_lm else 0.0)
    idx, ln, sc = _beam(lib, R.pad(x, fl, "nan"), W, nbest, fl=fl, **kw)
    for b, tb in enumerate(fl):
        si, sl, ss = _beam(lib, x[b:b + 1, :tb], W, nbest, **kw)
        assert np.array_equal(ln[b], sl[0]) and np.array_equal(bits(sc[b]), bits(ss[0])), f"W={W} clip {b} (Tb = {tb}): lengths or scores differ from the solo launch"
        assert np.array_equal(idx[b, :, :tb], si[0]) and (idx[b, :, tb:] == -1).all(), f"W={W} clip {b} (Tb = {tb}): hypotheses differ"
        assert ln[b, 0] >= 0
    full = _beam(lib, x, W, nbest, **kw)                                 # today's entry point on the same batch: the clip with Tb = T
    b = int(np.nonzero(fl == T)[0][0])
    assert np.array_equal(idx[b], full[0][b]) and np.array_equal(ln[b], full[1][b]) and np.array_equal(bits(sc[b]), bits(full[2][b]))
    for lens in ("null", np.full(B, T, np.int32)):
        got = _beam(lib, x, W, nbest, fl=lens, **kw)
        assert all(np.array_equal(bits(g), bits(f)) for g, f in zip(got, full)), "without lengths the launch is not today's"
    fl_bad = fl.copy()
    fl_bad[[1, 3, 5, 7]] = (0, -3, T + 1, 2 ** 31 - 1)
    i2, l2, s2 = _beam(lib, R.pad(x, fl, "nan"), W, nbest, fl=fl_bad, **kw)
    for b in range(B):
        if b in (1, 3, 5, 7):
            assert (l2[b] == -1).all() and np.isneginf(s2[b]).all() and (i2[b] == -1).all()
        else:
            assert np.array_equal(i2[b], idx[b]) and np.array_equal(l2[b], ln[b]) and np.array_equal(bits(s2[b]), bits(sc[b]))


# ------------------------------------------------------------------ align
def _align(lib, x, y, blank, fl="fixed"):
    x, y = np.asarray(x, np.float32), np.asarray(y, np.int64)
    B, T, Cc = x.shape
    L = y.shape[1]
    bufs = dict(logits=Guarded.of(x), labels=Guarded.of(y), ws=Guarded(max(int(lib.ishara_ctc_align_workspace_bytes(B, T, L)), 16)),
                frame_pos=Guarded(4 * B * T, 0x7F), start=Guarded(4 * B * L, 0x7F), end=Guarded(4 * B * L, 0x7F), conf=Guarded(4 * B * L), score=Guarded(4 * B))
    if not isinstance(fl, str):
        bufs["frame_len"] = Guarded.of(np.asarray(fl, np.int32))
    p = {k: v.ptr() for k, v in bufs.items()}
    a = (p["logits"], p["labels"], B, T, Cc, L, blank, p["ws"], p["frame_pos"], p["start"], p["end"], p["conf"], p["score"])
    if isinstance(fl, str) and fl == "fixed":
        _lib.check(lib.ishara_ctc_align(*a, stream()), "ishara_ctc_align")
    else:
        _lib.check(lib.ishara_ctc_align_ex(*a, p.get("frame_len"), stream()), "ishara_ctc_align_ex")
    _finish(bufs)
    return (bufs["frame_pos"].get(torch.int32, B, T), bufs["start"].get(torch.int32, B, L), bufs["end"].get(torch.int32, B, L),
            bufs["conf"].get(torch.float32, B, L), bufs["score"].get(torch.float32, B))


def _check_align(lib, rc):
    x, y, fl = R.logits(rc), R.labels(rc), R.frame_len(rc)
    got = _align(lib, R.pad(x, fl, "nan"), y, rc.blank, fl)
    want = R.align_rows(x, y, fl, rc.blank)
    for k, name in enumerate(("frame_pos", "start", "end")):
        assert np.array_equal(got[k], want[k]), f"{rc.name}: {name} is not viterbi_align of the samples' own frames"
    ok = R.feasible(rc)
    assert (got[4][~ok] == np.float32(-1e30)).all() and not bits(got[3][~ok]).any()
    for b, tb in enumerate(fl):
        solo = _align(lib, x[b:b + 1, :tb], y[b:b + 1], rc.blank)
        assert np.array_equal(got[0][b, :tb], solo[0][0]) and np.array_equal(got[1][b], solo[1][0]) and np.array_equal(got[2][b], solo[2][0])
        assert np.array_equal(bits(got[3][b]), bits(solo[3][0])) and bits(got[4])[b] == bits(solo[4])[0], f"{rc.name}: sample {b} (Tb = {tb}): conf or score differ from the solo launch"
    return got


def test_align_with_lengths_back_pointers_in_lds(lib):
    rc = R.align_case(64)
    assert lib.ishara_ctc_align_workspace_bytes(rc.B, rc.T, rc.L) == 128
    got = _check_align(lib, rc)
    x, y, fl = R.logits(rc), R.labels(rc), R.frame_len(rc)
    full = _align(lib, x, y, rc.blank)
    for lens in ("null", np.full(rc.B, rc.T, np.int32)):
        again = _align(lib, x, y, rc.blank, lens)
        assert all(np.array_equal(bits(a), bits(f)) for a, f in zip(again, full)), "without lengths the launch is not today's"
    fl_bad = fl.copy()
    fl_bad[[1, 3, 5, 7]] = (0, -3, rc.T + 1, 2 ** 31 - 1)
    bad = _align(lib, R.pad(x, fl, "nan"), y, rc.blank, fl_bad)
    for b in range(rc.B):
        if b in (1, 3, 5, 7):
            assert (bad[0][b] == -1).all() and (bad[1][b] == -1).all() and (bad[2][b] == -1).all() and not bits(bad[3][b]).any() and bad[4][b] == np.float32(-1e30)
        else:
            assert all(np.array_equal(bits(p[b]), bits(q[b])) for p, q in zip(bad, got))


@pytest.mark.parametrize("k", [0, 1])
def test_align_with_lengths_back_pointers_in_the_workspace(lib, k):
    rc = R.align_case(1300)[k]
    assert lib.ishara_ctc_align_workspace_bytes(rc.B, rc.T, rc.L) == rc.B * rc.T * 128
    _check_align(lib, rc)


# ------------------------------------------------------------------ the Python surface
def _torch_ref(x, tg, il, tl, blank, reduction, zero_infinity, backward=True):
    xr = torch.from_numpy(x.astype(np.float64)).requires_grad_(backward)
    v = torch.nn.functional.ctc_loss(torch.log_softmax(xr, -1).transpose(0, 1), torch.from_numpy(tg), torch.tensor(il), torch.tensor(tl), blank, reduction, zero_infinity)
    if backward:
        v.sum().backward()
    return v.detach().numpy(), xr.grad.numpy() if backward else None


@pytest.mark.parametrize("reduction", ["none", "sum", "mean"])
@pytest.mark.parametrize("blank", [0, 16])
@pytest.mark.parametrize("zero_infinity", [False, True])
def test_python_ctc_loss_is_torch_ctc_loss(reduction, blank, zero_infinity):
    """loss and gradient with respect to x inside the ctc_parity bounds scaled by the reduction's per-sample weight; sample 2 is infeasible
    (6 symbols in 5 frames): with zero_infinity off only the loss (inf) is compared, torch's gradient there is not a contract"""
    g = np.random.default_rng([7, blank])
    B, T, Cc, S = 5, 21, 17, 8
    x = (2 * g.standard_normal((B, T, Cc))).astype(np.float32)
    il, tl = [21, 13, 5, 1, 20], [8, 4, 6, 0, 3]
    cls = np.array([c for c in range(Cc) if c != blank])
    tg = cls[g.integers(0, len(cls), (B, S))].astype(np.int64)
    tg[2, :6] = cls[np.arange(6) % 2]                                     # no repeats: infeasible only because 6 > 5
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    v = ishara_amd.ctc_loss(xd, torch.from_numpy(tg), torch.tensor(il, device="cuda"), tl, blank=blank, reduction=reduction, zero_infinity=zero_infinity)
    (v.sum() if reduction == "none" else v).backward()
    got, grad = v.detach().cpu().numpy().astype(np.float64), xd.grad.cpu().numpy().astype(np.float64)
    per, _ = _torch_ref(x, tg, il, tl, blank, "none", True, backward=False)
    w = 1.0 / (B * np.maximum(np.array(tl), 1)) if reduction == "mean" else np.ones(B)
    if not zero_infinity:
        want, _ = _torch_ref(x, tg, il, tl, blank, reduction, False, backward=False)
        if reduction == "none":
            ok = np.array([0, 1, 3, 4])
            assert np.isposinf(got[2]) and np.isposinf(want[2]) and (np.abs(got[ok] - want[ok]) <= P.NLL_ATOL + P.NLL_RTOL * np.abs(want[ok])).all()
        else:
            assert np.isposinf(got) and np.isposinf(want)
        return
    want, wg = _torch_ref(x, tg, il, tl, blank, reduction, True)
    if reduction == "none":
        assert (np.abs(got - want) <= P.NLL_ATOL + P.NLL_RTOL * np.abs(want)).all() and got[2] == 0
    else:
        assert abs(got - want) <= (w * (P.NLL_ATOL + P.NLL_RTOL * np.abs(per))).sum()
    assert (np.abs(grad - wg) <= w[:, None, None] * P.GRAD_ATOL + P.GRAD_RTOL * np.abs(wg)).all()
    assert not grad[2].any() and all(not grad[b, il[b]:].any() for b in range(B))
    if reduction == "sum":                                               # an incoming gradient other than 1
        xd.grad = None
        (3.0 * ishara_amd.ctc_loss(xd, torch.from_numpy(tg), il, tl, blank=blank, reduction="sum", zero_infinity=True)).backward()
        assert np.allclose(xd.grad.cpu().numpy(), 3.0 * grad, rtol=1e-6, atol=0)


GOLD = None


def _golden():
    import os
    global GOLD
    if GOLD is None:
        GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "squeezeformer_top.npz"))
    G = GOLD
    cfg = {str(k): int(v) for k, v in zip(G["cfg_keys"], G["cfg_vals"])}
    B, T, _ = G["x"].shape
    m = ishara_amd.Squeezeformer(cfg["num_classes"], cfg["input_dim"], cfg["encoder_dim"], cfg["num_encoder_layers"], cfg["reduce_layer_index"],
                                 cfg["recover_layer_index"], cfg["num_attention_heads"], cfg["feed_forward_expansion_factor"], cfg["conv_expansion_factor"],
                                 0.0, 0.0, 0.0, 0.0, cfg["conv_kernel_size"], bool(cfg["half_step_residual"]), seq_len=T, max_batch=B, dtype="f32")
    m.load_state_dict({k[3:]: torch.from_numpy(G[k]) for k in G.files if k.startswith("sd/")})
    return G, m


def test_pinned_fixture_loss_on_the_librarys_own_kernel():
    """the assertion tests/test_golden_squeezeformer_top_gpu.py makes with torch's kernel (on the training-mode log-probabilities, as
    there); the lengths go in as a device tensor and come out as one"""
    G, m = _golden()
    with torch.no_grad():
        y, yl = m.train()(torch.from_numpy(G["x"]), torch.from_numpy(G["lengths"]).cuda())
    assert yl.is_cuda and yl.tolist() == G["eval_len"].tolist()
    loss = ishara_amd.ctc_loss(y, torch.from_numpy(G["ctc_targets"]), yl, torch.tensor([5, 4]), blank=0, reduction="sum")
    assert abs(float(loss) - float(G["ctc_loss"])) <= 1e-3 * float(G["ctc_loss"])


def test_top_level_trains_on_the_librarys_own_loss():
    G, m = _golden()
    m.train()
    x, lens, tgt = torch.from_numpy(G["x"]).cuda(), torch.from_numpy(G["lengths"]), torch.from_numpy(G["ctc_targets"])
    opt = torch.optim.SGD(m.parameters(), lr=0.02)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        y, yl = m(x, lens)
        loss = ishara_amd.ctc_loss(y, tgt, yl, torch.tensor([5, 4]), blank=0, reduction="sum")
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


def test_model_methods_with_frame_lengths():
    """Model.decode_batch / beam_decode / align / ctc_loss with frame_lengths equal the per-clip sliced calls; with None they are today's"""
    m = ishara_amd.get_model(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(48, 36), dtype="f32", max_batch=4, device="cuda:0", seed=0)
    rc = R.Ragged("model", 48, 60, 12, 59, ((48, 9, (4,)), (17, 7, ()), (9, 12, ()), (30, 0, ())), seed=2700)
    x, y, fl = torch.from_numpy(R.logits(rc)).cuda(), R.labels(rc), R.frame_len(rc)
    xn = torch.from_numpy(R.pad(R.logits(rc), fl, "nan")).cuda()
    sl = [x[b:b + 1, :fl[b]].contiguous() for b in range(rc.B)]
    dec = m.decode_batch(xn, frame_lengths=fl)
    beam = m.beam_decode(xn, 8, 2, frame_lengths=torch.from_numpy(fl).cuda())
    al = m.align(xn, y, frame_lengths=list(fl))
    nll = m.ctc_loss(y, xn, frame_lengths=fl).cpu().numpy()
    for b in range(rc.B):
        assert np.array_equal(dec[b], m.decode_batch(sl[b])[0])
        one = m.beam_decode(sl[b], 8, 2)[0]
        assert len(beam[b]) == len(one) and all(np.array_equal(p, q) and s == t for (p, s), (q, t) in zip(beam[b], one))
        a1 = m.align(sl[b], y[b:b + 1])[0]
        assert np.array_equal(al[b].frame_pos[:fl[b]], a1.frame_pos) and (al[b].frame_pos[fl[b]:] == -1).all() and al[b].score == a1.score and al[b].spans == a1.spans
        assert bits(nll)[b] == bits(m.ctc_loss(y[b:b + 1], sl[b]).cpu().numpy())[0]
    assert nll[2] >= P.SENTINEL                                          # 12 symbols in 9 frames
    lib = _lib.load()
    assert same(m.ctc_loss(y, x).cpu().numpy(), loss_fixed(lib, R.logits(rc), y, rc.blank, grad=False)[0])
    assert all(np.array_equal(p, q) for p, q in zip(m.decode_batch(x), ishara_amd.ctc_greedy_decode(x)))
    assert all(np.array_equal(p.frame_pos, q.frame_pos) and p.score == q.score for p, q in zip(m.align(x, y), ishara_amd.ctc_align(x, y)))
    assert all(np.array_equal(p[0][0], q[0][0]) and p[0][1] == q[0][1] for p, q in zip(m.beam_decode(x, 8, 2), ishara_amd.ctc_beam_decode(x, None, 8, 2)))
