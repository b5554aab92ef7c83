"""The CTC loss kernel and the greedy decoder (csrc/ctc.hip) against fp64 at their layout edges: every register count and seam of the
register-resident lattice, frame-group tails, single-alignment and infeasible samples, class counts and blank indices, logit regimes,
grad_scale and the nll-only route, the packed bf16 copy of the gradient, memory discipline, out-of-range labels; the decoder bit-exactly on
run structure, round boundaries, ties and clamped loads.  Cases, references and bounds: tests/ctc_parity.py.

One launch per batch; every sample's nll and every element of dlogits is compared.  Every buffer of every launch lies between two guard
regions that must come back unchanged, and every output is pre-filled with 0xFF bytes (NaN): an element the kernel leaves out fails."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ctc_parity as P
from ishara_amd import _lib
from oracle import ishara_oracle as O

pytestmark = pytest.mark.gpu

GUARD = 4096          # bytes on either side of every buffer
GUARD_BYTE = 0xA5


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

    def view(self, dtype, *shape):
        return self.inner.view(dtype).view(*shape)

    def check(self, name):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == GUARD_BYTE).all() and (b[GUARD + self.n:] == GUARD_BYTE).all(), f"{name}: bytes outside the buffer were written"


def run_loss(lib, x, y, blank, gs=1.0, grad=True, dlb=False, op=False, ws_fill=0xFF):
    """one launch -> dict(nll [B] f32, grad [B,T,C] f32 or None, dlb [B*T,128] int16 bit patterns or None); the guards are checked"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.int64)
    B, T, Cc = x.shape
    L = y.shape[1]
    n_ws = int(lib.ishara_ctc_workspace_bytes(B, T, L))
    assert n_ws == 2 * B * T * 64 * ((2 * L + 1 + 63) // 64) * 8
    bufs = dict(logits=Guarded.of(x), labels=Guarded.of(y), nll=Guarded(4 * B), ws=Guarded(n_ws, ws_fill))
    if grad:
        bufs["dlogits"] = Guarded(4 * B * T * Cc)
    if dlb:
        bufs["dlb"] = Guarded(2 * B * T * 128)
    p = {k: v.ptr() for k, v in bufs.items()}
    if op or dlb:
        rc = lib.ishara_op_ctc_loss(p["logits"], p["labels"], B, T, Cc, L, blank, p["nll"], p.get("dlogits"), C.c_float(gs), p["ws"], p.get("dlb"), stream())
    else:
        rc = lib.ishara_ctc_loss(p["logits"], p["labels"], B, T, Cc, L, blank, p["nll"], p.get("dlogits"), C.c_float(gs), p["ws"], stream())
    _lib.check(rc, "ctc_loss")
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert torch.equal(bufs["logits"].view(torch.float32, B, T, Cc).cpu(), torch.from_numpy(x)) and torch.equal(bufs["labels"].view(torch.int64, B, L).cpu(), torch.from_numpy(y))
    return dict(nll=bufs["nll"].view(torch.float32, B).cpu().numpy(),
                grad=bufs["dlogits"].view(torch.float32, B, T, Cc).cpu().numpy() if grad else None,
                dlb=bufs["dlb"].view(torch.int16, B * T, 128).cpu().numpy() if dlb else None)


def run_case(lib, case, **kw):
    return run_loss(lib, P.logits(case), P.labels(case), case.blank, **kw)


def _log(case, obs, **extra):
    """observed err / bound per quantity: printed, and appended to the file ISHARA_CTC_LOG names (DESIGN.md §2 quotes them)"""
    print(case.name, {k: f"{v:.3g}" for k, v in obs.items()}, extra or "")
    path = os.environ.get("ISHARA_CTC_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(dict(case=case.name, regime=case.regime, B=case.B, T=case.T, C=case.C, L=case.L, **obs, **extra)) + "\n")


def check(case, out, gs=1.0, ref=None, **extra):
    obs, bad = P.compare(case, out["nll"], out["grad"], gs, ref)
    _log(case, obs, grad_scale=gs, **extra)
    assert not bad, bad
    return obs


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def check_dlb(out, Cc):
    """dlb is dlogits rounded to bf16 in columns < C and +0 in columns C .. 127, every row"""
    want = torch.from_numpy(out["grad"]).reshape(-1, Cc).to(torch.bfloat16).view(torch.int16).numpy()
    assert np.array_equal(out["dlb"][:, :Cc], want), "dlb is not the bf16 rounding of dlogits"
    assert not out["dlb"][:, Cc:].any(), "dlb columns C..127 are not zero"


# ------------------------------------------------------------------ A: register counts and seams
@pytest.mark.parametrize("L,ns", list(zip(P.A_LS, P.A_NS)))
def test_register_counts_and_seams(lib, L, ns):
    """ctc_kernel<NS> for NS = 1 .. 8 with lattices ending on either side of every register seam (NK = 1, 2 and the run-time count), labels
    equal and different across each seam.  (Two fp64 lattices of 64 NS states per frame: 1024 NS bytes per sample and frame.)"""
    assert lib.ishara_ctc_workspace_bytes(1, 1, L) // 512 == 2 * ns
    case = P.case_a(L)
    assert P.feasible(case).all() and P.lengths(case)[1].max() <= 6
    check(case, run_case(lib, case))


# ------------------------------------------------------------------ B: frame tails
@pytest.mark.parametrize("T", P.B_TS)
@pytest.mark.parametrize("L", [8, 64])
def test_frame_group_tails(lib, L, T):
    """the 8-frame gather / settle groups start at t = 1 and the gradient phase strides 16 frames per wave"""
    case = P.case_b(L, T)
    assert P.feasible(case).all()
    check(case, run_case(lib, case))


# ------------------------------------------------------------------ C: one alignment only
@pytest.mark.parametrize("i", range(len(P.TIGHT)), ids=lambda i: "len%d-rep%d" % (P.TIGHT[i][0], len(P.TIGHT[i][1])))
def test_single_alignment(lib, i):
    case = P.case_c(i)
    out = run_case(lib, case)
    check(case, out)
    check(case, out, ref=P.closed_form(case), reference="closed form")


# ------------------------------------------------------------------ D: infeasible samples
@pytest.mark.parametrize("i", P.D_IS, ids=lambda i: "len%d-rep%d" % (P.TIGHT[i][0], len(P.TIGHT[i][1])))
def test_infeasible_sample_and_its_neighbours(lib, i):
    case = P.case_d(i)
    ok = P.feasible(case)
    assert not ok[1] and ok[[0, 2, 3]].all()
    out = run_case(lib, case, gs=0.5, dlb=True)
    assert out["nll"][1] >= P.SENTINEL and np.isfinite(out["grad"][1]).all()
    obs = check(case, out, gs=0.5)
    assert "grad_infeasible" in obs
    check_dlb(out, case.C)
    y2 = P.labels(case).copy()
    y2[1, :] = case.blank
    alone = run_loss(lib, P.logits(case), y2, case.blank, gs=0.5, dlb=True)
    T = case.T
    for b in (0, 2, 3):
        assert bits(out["nll"])[b] == bits(alone["nll"])[b]
        assert np.array_equal(bits(out["grad"][b]), bits(alone["grad"][b]))
        assert np.array_equal(out["dlb"][b * T:(b + 1) * T], alone["dlb"][b * T:(b + 1) * T])


# ------------------------------------------------------------------ E: classes and blank
@pytest.mark.parametrize("Cc,blank", P.E_CB)
def test_class_counts_and_blank_index(lib, Cc, blank):
    case = P.case_e(Cc, blank)
    y = P.labels(case)
    assert ((y >= 0) & (y < Cc)).all() and P.feasible(case)[:2].all()
    assert P.feasible(case).all() == (Cc > 2)          # one label class: every label repeats its neighbour, 31 symbols need 61 frames
    check(case, run_case(lib, case))


# ------------------------------------------------------------------ F: logit regimes
@pytest.mark.parametrize("regime", [r for r in P.REGIMES if r != "n2"])
@pytest.mark.parametrize("L,T", P.F_SHAPES)
def test_logit_regimes(lib, L, T, regime):
    case = P.case_f(L, T, regime)
    assert P.feasible(case).all()
    check(case, run_case(lib, case))


# ------------------------------------------------------------------ G: scale and nll-only
def test_grad_scale_and_nll_only(lib):
    case = P.case_g()
    one = run_case(lib, case)
    check(case, one)
    quarter = run_case(lib, case, gs=0.25)
    assert np.array_equal(bits(quarter["grad"]), bits(np.float32(0.25) * one["grad"])) and np.array_equal(bits(quarter["nll"]), bits(one["nll"]))
    check(case, run_case(lib, case, gs=37.5), gs=37.5)
    only = run_case(lib, case, grad=False)
    assert np.array_equal(bits(only["nll"]), bits(one["nll"]))
    check(case, only)


# ------------------------------------------------------------------ H: the packed bf16 copy
@pytest.mark.parametrize("infeasible", [False, True])
@pytest.mark.parametrize("T", [9, 57])
@pytest.mark.parametrize("Cc", [60, 64, 33])
def test_bf16_copy_of_the_gradient(lib, Cc, T, infeasible):
    case = P.case_h(Cc, T, infeasible)
    assert P.feasible(case).all() != infeasible
    out = run_case(lib, case, gs=1 / 64, dlb=True)
    check(case, out, gs=1 / 64)
    check_dlb(out, Cc)
    plain = run_case(lib, case, gs=1 / 64)              # the entry point without dlb computes the same
    assert np.array_equal(bits(plain["grad"]), bits(out["grad"])) and np.array_equal(bits(plain["nll"]), bits(out["nll"]))


# ------------------------------------------------------------------ I: memory discipline
@pytest.mark.parametrize("case", [P.case_a(32), P.case_a(255), P.case_b(8, 9), P.case_b(64, 9)], ids=lambda c: c.name)
def test_memory_discipline(lib, case):
    """ws at exactly ishara_ctc_workspace_bytes needs no initialisation; nothing outside the documented extents is written (run_loss checks
    the guards of every buffer); the gradient of a frame sums to 0 and never exceeds the softmax"""
    ff = run_case(lib, case, dlb=True, ws_fill=0xFF)
    zz = run_case(lib, case, dlb=True, ws_fill=0x00)
    for k in ("nll", "grad", "dlb"):
        assert np.array_equal(bits(ff[k]), bits(zz[k])), f"{k} depends on what the workspace held"
    check(case, ff)
    check_dlb(ff, case.C)
    g = ff["grad"].astype(np.float64)
    assert np.abs(g.sum(-1)).max() <= case.C * P.GRAD_ATOL
    assert (P.softmax64(P.logits(case)) - g).min() >= -P.GRAD_ATOL


# ------------------------------------------------------------------ J: batch
@pytest.mark.parametrize("B", [1, 300])
def test_batch_sizes(lib, B):
    case = P.case_j(B)
    check(case, run_case(lib, case))


# ------------------------------------------------------------------ K: out-of-range labels
@pytest.mark.parametrize("Cc,value,pos", [(60, 60, 3), (60, 63, 0), (60, -1, 6), (33, 33, 3), (33, 63, 6), (33, -1, 0), (5, 5, 0), (5, 40, 3), (5, -1, 6)])
def test_out_of_range_label(lib, Cc, value, pos):
    """a label outside [0, C) makes its sample infeasible and is never used as an index; the logits lie inside a larger allocation (run_loss:
    4 KiB on either side), so that a kernel indexing with such a value would still stay within allocated memory"""
    case = P.case_k(Cc, value, pos)
    y = P.labels(case)
    assert y[1, pos] == value and not P.feasible(case)[1] and P.feasible(case)[[0, 2, 3]].all()
    out = run_case(lib, case, gs=0.5, dlb=True)
    assert out["nll"][1] >= P.SENTINEL and np.isfinite(out["grad"][1]).all()
    check(case, out, gs=0.5)
    check_dlb(out, Cc)
    y2 = y.copy()
    y2[1, :] = case.blank
    alone = run_loss(lib, P.logits(case), y2, case.blank, gs=0.5, dlb=True)
    T = case.T
    for b in (0, 2, 3):
        assert bits(out["nll"])[b] == bits(alone["nll"])[b] and np.array_equal(bits(out["grad"][b]), bits(alone["grad"][b]))
        assert np.array_equal(out["dlb"][b * T:(b + 1) * T], alone["dlb"][b * T:(b + 1) * T])


# ------------------------------------------------------------------ greedy decode
DECODE_TS = (1, 2, 3, 255, 256, 257, 258, 511, 512, 513, 4096)
DECODE_CS = (1, 2, 15, 16, 17, 60, 64, 65, 100)


def _from_argmax(g, a, Cc, shift=0.0):
    """logits [T, C] whose argmax sequence is `a`: a margin of 1 over N(0, 0.01^2) noise"""
    x = (0.01 * g.standard_normal((len(a), Cc)) + shift).astype(np.float32)
    x[np.arange(len(a)), a] = np.float32(1.0 + shift)
    return x


def decode_batch(T, Cc, blank, seed):
    """[n, T, C] float32: one row per pattern"""
    g = np.random.default_rng([3, T, Cc, blank, seed])
    t = np.arange(T)
    nb = [c for c in range(Cc) if c != blank] or [0]
    two = (nb * 2)[:2]
    rows = []
    rows.append(_from_argmax(g, np.array(two)[t % 2], Cc))                               # alternating classes: every frame but the last is kept
    rows.append(_from_argmax(g, np.full(T, nb[-1]), Cc))                                 # constant: empty decode
    rows.append(_from_argmax(g, np.full(T, blank), Cc))
    runs = []
    while len(runs) < T:                                                                 # runs of 1 .. 5 frames, blanks between and inside
        runs += [int(g.choice([blank, nb[g.integers(len(nb))]]))] * int(g.integers(1, 6))
    rows.append(_from_argmax(g, np.array(runs[:T]), Cc))
    rows.append(_from_argmax(g, np.array(runs[:T]), Cc, shift=-50.0))                    # all-negative logits
    seg = (t >= 256).astype(int) + (t >= 257) + (t >= 512)                               # a change exactly at 255|256, 256|257 and 511|512
    rows.append(_from_argmax(g, np.array((nb * 4)[:4])[seg] if len(nb) > 1 else np.where(seg % 2 == 0, nb[0], blank), Cc))
    seg = (t >= 255).astype(int) + (t >= 258) + (t >= 511) + (t >= 513)                  # changes around the round boundaries, none at them
    rows.append(_from_argmax(g, np.array((nb * 5)[:5])[seg] if len(nb) > 1 else np.where(seg % 2 == 0, nb[0], blank), Cc))
    rows.append(_from_argmax(g, np.where(t % 2 == 0, 0, Cc - 1), Cc))                    # the maximum in class 0 / in class C-1 (the clamped loads)
    rows.append(_from_argmax(g, np.where((t // 3) % 2 == 0, Cc - 1, 0), Cc))
    x = _from_argmax(g, np.array(runs[:T]), Cc)                                          # exact two-way ties: the first index wins
    lo, hi = t % Cc, (7 * t + 3) % Cc
    x[t, lo] = np.float32(2.0)
    x[t, hi] = np.float32(2.0)
    rows.append(x)
    x = _from_argmax(g, np.array(runs[:T]), Cc)                                          # all-way ties on every other pair of frames: class 0
    x[(t // 2) % 2 == 0, :] = np.float32(0.25)
    rows.append(x)
    return np.stack(rows)


@pytest.mark.parametrize("Cc,blank", sorted({(c, b) for c in DECODE_CS for b in (0, c - 1, c // 2)}))
def test_greedy_decode_is_decode_phrase(lib, Cc, blank):
    """bit-exact against decode_phrase: the whole out_idx row with its -1 padding, and out_len"""
    for T in DECODE_TS:
        x = decode_batch(T, Cc, blank, 0)
        B = x.shape[0]
        xd, idx, ln = Guarded.of(x), Guarded(4 * B * T), Guarded(4 * B)
        _lib.check(lib.ishara_greedy_decode(xd.ptr(), B, T, Cc, blank, idx.ptr(), ln.ptr(), stream()), "ishara_greedy_decode")
        torch.cuda.synchronize()
        for name, gd in (("logits", xd), ("out_idx", idx), ("out_len", ln)):
            gd.check(name)
        got, n = idx.view(torch.int32, B, T).cpu().numpy(), ln.view(torch.int32, B).cpu().numpy()
        for b in range(B):
            want = O.decode_phrase(x[b], blank)
            row = np.full(T, -1, np.int64)
            row[:len(want)] = want
            assert n[b] == len(want) and np.array_equal(got[b], row), f"T={T} C={Cc} blank={blank} pattern {b}: decode differs"
        if Cc >= 3:
            assert n[0] == T - 1                              # alternating: n = T - 1
        assert n[1] == 0 and n[2] == 0
        if T == 4096 and Cc >= 5:
            assert n[5] == 3 and n[6] == 4, (n[5], n[6])
        if Cc >= 2:
            assert ((x[9] == x[9].max(-1, keepdims=True)).sum(-1) == 2).any() and (x[10] == x[10].max(-1, keepdims=True)).all(-1).any()
