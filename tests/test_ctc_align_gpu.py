"""GPU: ishara_ctc_align (csrc/ctc_align.hip) against the host reference ishara_amd/ctc_align.py.  The semantics make the device result an
exact function of the inputs, so frame_pos, start and end are compared with == on every sample of every case: the register seams of the
lattice, the frame-group edges, single-alignment and infeasible samples, class counts and blank indices, logit regimes, exact ties, both
homes of the back-pointers (LDS and the caller's workspace).  conf and score are held to bounds derived from the number formats.

Every launch goes through the C ABI.  Every buffer lies between two guard regions that must come back unchanged; every output is pre-filled
with 0xFF bytes, so an element the kernel leaves out fails.  One launch and one reference per case, shared by the tests that need them."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ctc_parity as P
from ishara_amd import _lib, get_model
from ishara_amd.ctc_align import BP_ROW_BYTES, viterbi_align

pytestmark = pytest.mark.gpu

GUARD, GUARD_BYTE = 4096, 0xA5
CONF_ATOL = 1e-5                      # a mean of fp32 softmax values <= 1, each a handful of fp32 roundings over at most 64 terms
SCORE_PER_FRAME, SCORE_RTOL = 5e-6, 1e-12      # logf of a sum in [1, 64] in fp32: ~4e-6 per frame; everything else is fp64


def _stream():
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


def in_lds(lib, T, L):
    """the back-pointers of a (T, L) launch stay in LDS: the workspace is one untouched row"""
    return int(lib.ishara_ctc_align_workspace_bytes(1, T, L)) == BP_ROW_BYTES


def run_align(lib, x, y, blank, ws_fill=0xFF):
    """one launch -> (frame_pos [B,T], start [B,L], end [B,L] int32, conf [B,L], score [B] f32); guards, inputs and the workspace's use checked"""
    x, y = np.array(x, np.float32), np.array(y, np.int64)          # copies: the cases' arrays are read-only
    B, T, Cc = x.shape
    L = y.shape[1]
    n_ws = int(lib.ishara_ctc_align_workspace_bytes(B, T, L))
    assert n_ws == (BP_ROW_BYTES if in_lds(lib, T, L) else B * T * BP_ROW_BYTES)
    bufs = dict(logits=Guarded.of(x), labels=Guarded.of(y), ws=Guarded(n_ws, ws_fill), frame_pos=Guarded(4 * B * T), start=Guarded(4 * B * L),
                end=Guarded(4 * B * L), conf=Guarded(4 * B * L), score=Guarded(4 * B))
    p = {k: v.ptr() for k, v in bufs.items()}
    _lib.check(lib.ishara_ctc_align(p["logits"], p["labels"], B, T, Cc, L, blank, p["ws"], p["frame_pos"], p["start"], p["end"], p["conf"], p["score"],
                                    _stream()), "ishara_ctc_align")
    torch.cuda.synchronize()
    for k, v in bufs.items():
        v.check(k)
    assert torch.equal(bufs["logits"].view(torch.float32, B, T, Cc).cpu(), torch.from_numpy(x)) and torch.equal(bufs["labels"].view(torch.int64, B, L).cpu(), torch.from_numpy(y))
    if in_lds(lib, T, L):
        assert (bufs["ws"].inner == ws_fill).all(), "the workspace was written although the back-pointers fit in LDS"
    return (bufs["frame_pos"].view(torch.int32, B, T).cpu().numpy(), bufs["start"].view(torch.int32, B, L).cpu().numpy(),
            bufs["end"].view(torch.int32, B, L).cpu().numpy(), bufs["conf"].view(torch.float32, B, L).cpu().numpy(), bufs["score"].view(torch.float32, B).cpu().numpy())


@functools.lru_cache(maxsize=None)
def reference(case):
    return viterbi_align(P.logits(case), P.labels(case), case.blank)


@functools.lru_cache(maxsize=None)
def device(case):
    return run_align(_lib.load(), P.logits(case), P.labels(case), case.blank)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_exact(name, got, ref):
    """frame_pos, start, end: == on every sample"""
    for k, q in enumerate(("frame_pos", "start", "end")):
        if not np.array_equal(got[k], ref[k]):
            b = int(np.nonzero((got[k] != ref[k]).any(axis=1))[0][0])
            raise AssertionError(f"{name}: {q} of sample {b} differs\n device {got[k][b].tolist()}\n host   {ref[k][b].tolist()}")


def value_ratios(got, ref, T):
    """worst |err| / bound of conf and of score (<= 1 passes); a value that is not finite counts as an infinite error.  A sample without an
    alignment is held to its constants instead, bit for bit: score -1e30 (as fp32), conf 0"""
    conf, score = got[3].astype(np.float64), got[4].astype(np.float64)
    none = ref[4] == -1e30
    assert np.array_equal(bits(got[4][none]), bits(np.full(none.sum(), -1e30, np.float32))) and not got[3][none].any()
    rc = np.where(np.isfinite(conf), np.abs(conf - ref[3]) / CONF_ATOL, np.inf)
    rs = np.where(np.isfinite(score), np.abs(score - ref[4]) / (SCORE_PER_FRAME * T + SCORE_RTOL * np.abs(ref[4])), np.inf)
    return float(rc.max()), float(np.where(none, 0.0, rs).max())


K_ARGS = ((60, 60, 3), (60, 63, 0), (60, -1, 6), (33, 33, 3), (33, 63, 6), (33, -1, 0), (5, 5, 0), (5, 40, 3), (5, -1, 6))
CASES = ([P.case_a(L) for L in (31, 32, 63, 64, 255)]                                   # register seams at S = 63, 65, 127, 129, 511
         + [P.case_b(L, T) for L in (8, 64) for T in P.B_TS]                            # T = 1 and the emission group edges 8/9, 16/17
         + [P.case_c(i) for i in range(len(P.TIGHT))]                                   # one alignment, repeats across a seam
         + [P.case_d(i) for i in P.D_IS]                                                # infeasible between feasible
         + [P.case_e(Cc, blank) for Cc, blank in P.E_CB]
         + [P.case_f(64, 96, r) for r in P.REGIMES] + [P.case_f(255, 272, "n12")]
         + [P.case_g()] + [P.case_j(B) for B in (1, 3, 300)] + [P.case_k(*a) for a in K_ARGS])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_integer_outputs_equal_the_host_reference(lib, case):
    got, ref = device(case), reference(case)
    assert_exact(case.name, got, ref)
    ok = P.feasible(case)
    assert (ref[4][~ok] == -1e30).all() and (ref[4][ok] > -1e29).all()          # the two feasibility rules agree on these cases


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_conf_and_score_within_their_bounds(lib, case):
    got, ref = device(case), reference(case)
    ok = P.feasible(case)
    rc, rs = value_ratios(got, ref, case.T)
    print(f"{case.name}: conf err / bound = {rc:.3g}, score err / bound = {rs:.3g}")
    assert rc <= 1.0 and rs <= 1.0, (rc, rs)
    for b in range(case.B):          # past the label: exactly 0
        n = int(P.lengths(case)[0][b]) if ok[b] else 0
        assert not got[3][b, n:].any()


# ------------------------------------------------------------------ ties
TIES = P.Case("ties", 80, 60, 33, 59, ((33, ()), (33, (32,)), (20, (5,)), (1, ()), (0, ())), seed=1100)


@pytest.mark.parametrize("kind", ["zero", "integer"])
def test_exact_ties_follow_the_tie_order(lib, kind):
    """all-zero logits: every path ties; logits rounded to integers: sums of small integers tie exactly, many times per lattice"""
    y = P.labels(TIES)
    x = np.zeros((TIES.B, TIES.T, TIES.C), np.float32) if kind == "zero" else np.round(P.logits(TIES))
    got, ref = run_align(lib, x, y, TIES.blank), viterbi_align(x, y, TIES.blank)
    assert_exact(f"ties-{kind}", got, ref)
    assert max(value_ratios(got, ref, TIES.T)) <= 1.0
    if kind == "zero":          # stay > s-1 > s-2 from the end S-1: the shortest alignment first, then blanks
        n, rep = P.lengths(TIES)
        for b in range(TIES.B):
            tight = P.path_of(y[b], n[b], TIES.blank, n[b] + rep[b])
            emitted = np.nonzero(tight != TIES.blank)[0]
            assert got[1][b, :n[b]].tolist() == emitted.tolist() and got[2][b, :n[b]].tolist() == (emitted + 1).tolist()


# ------------------------------------------------------------------ the two homes of the back-pointers
def _edge_frames(lib, L):
    """the last T whose back-pointers fit in LDS at label capacity L, and the first that needs the workspace"""
    lo, hi = 1, 4096
    assert in_lds(lib, lo, L) and not in_lds(lib, hi, L)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if in_lds(lib, mid, L) else (lo, mid)
    return lo, hi


def _long_batch(T, L, seed):
    """two samples: a full-length label with repeats across two seams, a shorter one; random logits with +4 on a stretched alignment, so that
    the path wanders through the whole lattice"""
    case = P.Case(f"long-T{T}", T, 60, L, 59, ((L, tuple(p for p in (32, 64, 100) if p < L)), (min(L, 100), (7,))), regime="n2", seed=seed)
    y, n = P.labels(case), P.lengths(case)[0]
    x = P.logits(case).copy()
    for b in range(case.B):
        x[b, np.arange(T), P.path_of(y[b], n[b], case.blank, T)] += 4
    return x, y, case.blank


@pytest.mark.parametrize("which", ["lds_default_last", "lds_raised_first", "lds_last", "workspace_first", "T4096"])
def test_back_pointers_in_lds_and_in_the_workspace(lib, which):
    """T * 128 bytes of back-pointers: within the 64 KiB every launch is granted, above it (the raised limit) up to the last T that fits, then
    in the workspace: the first such T and the largest one the entry point takes, at L = 255"""
    L = 255
    last, first = _edge_frames(lib, L)
    default_last = (65536 - 512 - 256 * 8) // (BP_ROW_BYTES + 8)          # (m_t, sum_t) and the back-pointer row per frame, ext, the static part
    T = dict(lds_default_last=default_last, lds_raised_first=default_last + 1, lds_last=last, workspace_first=first, T4096=4096)[which]
    assert in_lds(lib, T, L) == (which.startswith("lds")) and default_last < last
    x, y, blank = _long_batch(T, L, 1200 + T)
    got, ref = run_align(lib, x, y, blank), viterbi_align(x, y, blank)
    assert (ref[4] > -1e29).all()
    assert_exact(which, got, ref)
    rc, rs = value_ratios(got, ref, T)
    print(f"{which} T={T}: conf err / bound = {rc:.3g}, score err / bound = {rs:.3g}")
    assert rc <= 1.0 and rs <= 1.0, (rc, rs)


# ------------------------------------------------------------------ isolation, determinism
@pytest.mark.parametrize("case", [P.case_d(5), P.case_d(9), P.case_k(60, 63, 0), P.case_k(5, -1, 6)], ids=lambda c: c.name)
def test_an_infeasible_sample_leaves_its_neighbours_alone(lib, case):
    ok = P.feasible(case)
    assert not ok[1] and ok[[0, 2, 3]].all()
    y = P.labels(case).copy()
    y[1, :] = case.blank
    got, alone = device(case), run_align(lib, P.logits(case), y, case.blank)
    for b in (0, 2, 3):
        for a, c in zip(got, alone):
            assert np.array_equal(bits(a[b]), bits(c[b]))
    assert (got[0][1] == -1).all() and (got[1][1] == -1).all() and (got[2][1] == -1).all() and not got[3][1].any() and got[4][1] == np.float32(-1e30)


@pytest.mark.parametrize("case", [P.case_a(64), P.case_f(255, 272, "n12")], ids=lambda c: c.name)
def test_two_launches_give_equal_bytes_whatever_the_workspace_held(lib, case):
    again = run_align(lib, P.logits(case), P.labels(case), case.blank, ws_fill=0x00)
    for a, c in zip(device(case), again):
        assert np.array_equal(bits(a), bits(c))


def test_graph_capture_equals_eager_and_an_empty_batch_is_a_no_op(lib):
    case = P.case_f(64, 96, "trained")
    x, y = torch.from_numpy(P.logits(case).copy()).cuda(), torch.from_numpy(P.labels(case).copy()).cuda()
    B, T, Cc, L = case.B, case.T, case.C, case.L
    ws = torch.empty(int(lib.ishara_ctc_align_workspace_bytes(B, T, L)), dtype=torch.uint8, device="cuda")
    outs = [torch.empty(s, dtype=d, device="cuda") for s, d in (((B, T), torch.int32), ((B, L), torch.int32), ((B, L), torch.int32), ((B, L), torch.float32), ((B,), torch.float32))]

    def run():
        _lib.check(lib.ishara_ctc_align(_lib.ptr(x), _lib.ptr(y), B, T, Cc, L, case.blank, _lib.ptr(ws), *[_lib.ptr(o) for o in outs], _stream()), "ishara_ctc_align")
    run()
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    for a, c in zip(eager, device(case)):
        assert np.array_equal(bits(a.cpu().numpy()), bits(c))
    for o in outs:
        o.view(torch.uint8).fill_(0xFF)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    torch.cuda.synchronize()
    for a, c in zip(eager, outs):
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    assert lib.ishara_ctc_align(None, None, 0, T, Cc, L, case.blank, None, None, None, None, None, None, _stream()) == 0


# ------------------------------------------------------------------ end to end
def test_model_align_equals_the_host_reference_on_the_models_logits():
    model = get_model(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(176, 276), dtype="f32", max_batch=4, seed=5)
    g = np.random.default_rng(77)
    logits = model(g.standard_normal((4, 176, 276)).astype(np.float32))
    y = np.full((4, 64), 59, np.int64)
    for b, n in enumerate((12, 1, 40, 0)):
        y[b, :n] = g.integers(0, 59, n)
    got = model.align(logits, y)
    ref = viterbi_align(logits.cpu().numpy(), y, 59)
    assert len(got) == 4 and (ref[4] > -1e29).all()
    for b, a in enumerate(got):
        n = int((y[b] != 59).sum())
        assert np.array_equal(a.frame_pos, ref[0][b]) and a.frame_pos.dtype == np.int32
        assert [(s[0], s[1], s[2]) for s in a.spans] == [(int(y[b, i]), int(ref[1][b, i]), int(ref[2][b, i])) for i in range(n)]
        assert np.abs(np.array([s[3] for s in a.spans]) - ref[3][b, :n]).max(initial=0.0) <= CONF_ATOL
        assert abs(a.score - ref[4][b]) <= SCORE_PER_FRAME * 176 + SCORE_RTOL * abs(ref[4][b])
    again = model.align(logits, y)          # the cached workspace
    assert all(np.array_equal(a.frame_pos, c.frame_pos) and a.spans == c.spans and a.score == c.score for a, c in zip(got, again))
