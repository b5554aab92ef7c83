"""CPU: the host reference of the CTC forced alignment (ishara_amd/ctc_align.py) against brute force over every frame string of tiny
lattices (optimal score, and the path the tie order selects), its structural properties on the cases of tests/ctc_parity.py, the closed
form of the tie order on all-zero logits, the refusals of ishara_ctc_align (NULL pointers: a refused call dereferences nothing) and
evaluation.alignment_table."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ctc_parity as P
from ishara_amd import ctc_align
from ishara_amd.ctc_align import Alignment, viterbi_align
from ishara_amd.evaluation import alignment_table

N = None


# ------------------------------------------------------------------ brute force over all C^T frame strings
def _collapse(string, blank):
    out, prev = [], None
    for c in string:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


def _strings_by_label(T, Cc, blank):
    """label (tuple) -> [n, T] array of every frame string that collapses to it"""
    groups = {}
    for s in itertools.product(range(Cc), repeat=T):
        groups.setdefault(_collapse(s, blank), []).append(s)
    return {k: np.array(v, np.int64) for k, v in groups.items()}


def _scalar_viterbi(x, lab, blank):
    """the semantics of the module docstring once more, state by state in plain Python -> the state path [T] (None: no alignment)"""
    T, n = x.shape[0], len(lab)
    S = 2 * n + 1
    ext = [blank if s % 2 == 0 else lab[s // 2] for s in range(S)]
    dead = -np.inf
    v = [np.float64(x[0, ext[s]]) if s < 2 else dead for s in range(S)]
    bp = [[0] * S for _ in range(T)]
    for t in range(1, T):
        new = []
        for s in range(S):
            best, b = v[s], 0
            if s >= 1 and v[s - 1] > best:
                best, b = v[s - 1], 1
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] and v[s - 2] > best:
                best, b = v[s - 2], 2
            new.append(best + np.float64(x[t, ext[s]]))
            bp[t][s] = b
        v = new
    s = S - 1
    if n > 0 and v[S - 2] > v[S - 1]:
        s = S - 2
    if v[s] == dead:
        return None
    path = [0] * T
    for t in range(T - 1, -1, -1):
        path[t] = s
        s = max(s - bp[t][s], 0)
    return path


def test_reference_is_brute_force_optimal_and_follows_the_tie_order():
    Cc = 4
    g = np.random.default_rng(2025)
    groups = {(T, blank): _strings_by_label(T, Cc, blank) for T in range(1, 7) for blank in (0, 3)}
    tied = infeasible = 0
    for it in range(240):
        T, blank, n = int(g.integers(1, 7)), (0, 3)[it % 2], int(g.integers(0, 4))
        cls = [c for c in range(Cc) if c != blank]
        lab = [cls[int(g.integers(3))] for _ in range(n)]
        L = n + int(g.integers(1, 3))
        y = np.array(lab + [blank] * (L - n), np.int64)
        x = (2 * g.standard_normal((T, Cc))).astype(np.float32)
        if it % 3 == 0:
            x = np.round(x)                                      # small integers: exact ties
        fp, st, en, cf, sc = viterbi_align(x, y, blank)
        cand = groups[T, blank].get(tuple(lab))
        if cand is None:                                         # no frame string spells the label
            infeasible += 1
            assert sc == -1e30 and (fp == -1).all() and (st == -1).all() and (en == -1).all() and not cf.any()
            assert _scalar_viterbi(x, lab, blank) is None
            continue
        V = np.zeros(len(cand))
        for t in range(T):                                       # the recursion's order of additions
            V = V + x[t, cand[:, t]].astype(np.float64)
        string = np.array([blank if i < 0 else lab[i] for i in fp])
        mine = np.nonzero((cand == string).all(axis=1))[0]
        assert mine.size == 1, "the path does not spell the label"
        assert V[mine[0]] == V.max(), (it, V[mine[0]], V.max())
        n_best = int((V == V.max()).sum())
        tied += n_best > 1
        states = _scalar_viterbi(x, lab, blank)
        assert fp.tolist() == [s >> 1 if s & 1 else -1 for s in states], it      # among tied optima: the one the tie order selects
        lp = x.astype(np.float64) - np.log(np.exp(x.astype(np.float64)).sum(axis=1, keepdims=True))
        assert abs(sc - lp[np.arange(T), string].sum()) <= 1e-9
        assert abs(sc - max(lp[np.arange(T), c].sum() for c in cand)) <= 1e-9
    assert tied >= 10 and infeasible >= 10, (tied, infeasible)


# ------------------------------------------------------------------ structure on the ctc_parity cases
CASES = ([P.case_a(31), P.case_a(64)] + [P.case_f(64, 96, r) for r in P.REGIMES] + [P.case_c(i) for i in range(len(P.TIGHT))]
         + [P.case_d(i) for i in P.D_IS] + [P.case_k(60, 63, 0), P.case_k(33, -1, 0), P.case_k(5, 40, 3)])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_structure_of_the_alignment(case):
    x, y = P.logits(case), P.labels(case)
    fp, st, en, cf, sc = viterbi_align(x, y, case.blank)
    n, rep = P.lengths(case)
    ok = P.feasible(case)
    nll = P.reference(case)[0]
    for b in range(case.B):
        if not ok[b]:                                            # the contract of a sample without an alignment
            assert sc[b] == -1e30 and (fp[b] == -1).all() and (st[b] == -1).all() and (en[b] == -1).all() and not cf[b].any()
            continue
        f = fp[b]
        keep = np.concatenate([[True], f[1:] != f[:-1]]) & (f >= 0)
        assert f[keep].tolist() == list(range(n[b])), "collapsing frame_pos does not give the label back"
        assert (st[b, n[b]:] == -1).all() and (en[b, n[b]:] == -1).all() and not cf[b, n[b]:].any()
        prev_end = 0
        for i in range(n[b]):                                    # the spans partition the non-blank frames, in order
            assert prev_end <= st[b, i] < en[b, i] and (f[st[b, i]:en[b, i]] == i).all()
            if i > 0 and y[b, i] == y[b, i - 1]:
                assert st[b, i] > prev_end, "no blank frame between a repeated symbol"
            prev_end = en[b, i]
        assert (en[b, :n[b]] - st[b, :n[b]]).sum() == (f >= 0).sum()
        assert ((cf[b, :n[b]] > 0) & (cf[b, :n[b]] <= 1)).all()
        assert sc[b] <= -nll[b] + 1e-6                           # one path is no more likely than all of them
        if n[b] + rep[b] == case.T:                              # one alignment: the path and the whole probability
            string = np.where(f >= 0, y[b][np.maximum(f, 0)], case.blank)
            assert np.array_equal(string, P.path_of(y[b], n[b], case.blank, case.T))
            assert abs(sc[b] + nll[b]) <= 1e-6 * max(1.0, abs(nll[b]))
    one = viterbi_align(x[0], y[0], case.blank)                  # one clip: the same five arrays without the batch axis
    assert all(np.array_equal(a, c[0]) for a, c in zip(one, (fp, st, en, cf, sc)))


def test_the_label_ends_at_its_first_blank():
    case = P.case_g()
    x, y = P.logits(case), P.labels(case).copy()
    ref = viterbi_align(x, y, case.blank)
    y[2, 10] = case.blank                                        # sample 2: 16 symbols, cut to 10; what follows is ignored
    cut = viterbi_align(x, y, case.blank)
    y[2, 10:] = case.blank
    assert all(np.array_equal(a, c) for a, c in zip(cut, viterbi_align(x, y, case.blank)))
    assert cut[1][2, 9] >= 0 and (cut[1][2, 10:] == -1).all() and ref[1][2, 15] >= 0


def test_all_zero_logits_pin_the_tie_order():
    """every path ties at 0: from the end S-1 the backtrace stays as long as the state was alive a frame earlier, then steps s-1, then s-2;
    a state is first alive at the frame the shortest alignment reaches it, so the path is that alignment (len + repeats frames, one per
    symbol, a blank between repeats) followed by blanks"""
    case = P.Case("zero", 80, 60, 33, 59, ((33, ()), (33, (32,)), (20, (5,)), (1, ()), (0, ())), seed=1100)
    y = P.labels(case)
    fp, st, en, cf, sc = viterbi_align(np.zeros((case.B, case.T, case.C), np.float32), y, case.blank)
    n, rep = P.lengths(case)
    for b in range(case.B):
        tight = P.path_of(y[b], n[b], case.blank, n[b] + rep[b])
        want = np.full(case.T, -1)
        want[np.nonzero(tight != case.blank)[0]] = np.arange(n[b])
        assert fp[b].tolist() == want.tolist()
        assert (en[b, :n[b]] - st[b, :n[b]] == 1).all()
        np.testing.assert_allclose(cf[b, :n[b]], 1 / 60, rtol=1e-12)
        assert abs(sc[b] + 80 * np.log(60)) <= 1e-9


def test_argument_checks_of_the_python_side():
    with pytest.raises(ValueError):
        viterbi_align(np.zeros((2, 3, 4), np.float32), np.zeros((3, 2), np.int64), 3)
    with pytest.raises(ValueError):
        viterbi_align(np.zeros((3, 4), np.float32), np.zeros(2, np.int64), 4)
    for bad in (dict(C=1), dict(C=65), dict(T=0), dict(T=4097), dict(L=0), dict(L=256), dict(blank=60), dict(blank=-1)):
        with pytest.raises(ValueError):
            ctc_align.check_device_args(**{**dict(C=60, T=16, L=8, blank=59), **bad})
    ctc_align.check_device_args(C=60, T=4096, L=255, blank=0)


# ------------------------------------------------------------------ the C entry point: refused before any HIP call
NAME = "ishara_ctc_align"
PTRS = ("logits", "labels", "ws", "frame_pos", "start", "end", "conf", "score")


def _call(lib_, ptrs=None, **kw):
    """one call with made-up aligned addresses (a refused call dereferences nothing) or `ptrs`; the stream is NULL"""
    v = dict(B=2, T=16, C=60, L=8, blank=59)
    assert set(kw) <= set(v), kw
    v.update(kw)
    p = {k: C.c_void_p(4096 * (i + 1)) for i, k in enumerate(PTRS)}
    p.update(ptrs or {})
    return lib_.ishara_ctc_align(p["logits"], p["labels"], v["B"], v["T"], v["C"], v["L"], v["blank"], *[p[k] for k in PTRS[2:]], N)


def _refused(lib_, rc, *words):
    msg = (lib_.ishara_last_error() or b"").decode()
    assert rc != 0, "accepted the call"
    assert msg.startswith(NAME + ":"), f"the error is not the entry point's own refusal: {msg!r}"
    for w in words:
        assert w in msg, f"{msg!r} does not say {w!r}"


@pytest.mark.parametrize("kw,words", [(dict(B=-1), ("B=-1",)), (dict(T=0), ("T=0", "1..4096")), (dict(T=4097), ("T=4097", "1..4096")), (dict(T=-3), ("T=-3",)),
                                      (dict(L=0), ("L=0", "1..255")), (dict(L=256), ("L=256", "1..255")), (dict(C=1, blank=0), ("C=1", "2..64")),
                                      (dict(C=65, blank=64), ("C=65", "2..64")), (dict(blank=-1), ("blank -1", "0..59")), (dict(blank=60), ("blank 60", "0..59")),
                                      (dict(C=5, blank=5), ("blank 5", "0..4"))],
                         ids=lambda v: "-".join(f"{k}{x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_entry_point_refuses_shapes(lib, kw, words):
    _refused(lib, _call(lib, **kw), *words)
    _refused(lib, _call(lib, ptrs={k: N for k in PTRS}, **kw), *words)          # before it looks at a pointer


def test_entry_point_refuses_null_and_misaligned_buffers(lib):
    _refused(lib, _call(lib, ptrs={k: N for k in PTRS}), "null")
    for k in PTRS:
        _refused(lib, _call(lib, ptrs={k: N}), "null")
    for off in (1, 2, 4, 8):
        _refused(lib, _call(lib, ptrs=dict(ws=C.c_void_p(4096 * 3 + off))), "ws", "16-byte")


def test_an_empty_batch_is_a_no_op_and_the_workspace_size_follows_the_frame_count(lib):
    assert _call(lib, B=0, ptrs={k: N for k in PTRS}) == 0
    _refused(lib, _call(lib, B=0, L=300), "L=300")                  # the shape checks still hold
    wb = lib.ishara_ctc_align_workspace_bytes
    assert wb(0, 384, 64) == 0 and wb(256, 384, 64) == 128 and wb(2, 1, 1) == 128            # back-pointers in LDS: one untouched row
    assert wb(2, 4096, 255) == 2 * 4096 * 128 and wb(3, 4096, 1) == 3 * 4096 * 128           # in the workspace: 128 bytes per frame
    assert [wb(1, T, 255) > 128 for T in (384, 1024, 1400)] == [False, False, True]
    for bad in ((-1, 16, 8), (2, 0, 8), (2, 4097, 8), (2, 16, 0), (2, 16, 256)):
        assert wb(*bad) == -1
    assert ctc_align.workspace_bytes(lib, 2, 4096, 255) == 2 * 4096 * ctc_align.BP_ROW_BYTES
    with pytest.raises(ValueError):
        ctc_align.workspace_bytes(lib, 2, 5000, 8)


# ------------------------------------------------------------------ the text table
def test_alignment_table():
    num_to_char = {0: "a", 1: "b", 5: " "}
    a = Alignment(np.array([-1, 0, 0, 1, -1, 2, 2, 2], np.int32), -3.25, [(0, 1, 3, 0.875), (5, 3, 4, 0.5), (1, 5, 8, 0.0625)])
    lines = alignment_table(a, num_to_char).split("\n")
    assert len(lines) == 1 + 3 + 1 and lines[0].split() == ["#", "sym", "first", "last", "frames", "conf"]
    assert lines[1].split() == ["0", "a", "1", "2", "2", "0.875"]
    assert lines[2].split() == ["1", "3", "3", "1", "0.500"] and lines[2][4:7] == "   "      # a space stays a space
    assert lines[3].split() == ["2", "b", "5", "7", "3", "0.062"]
    assert lines[4] == "log p(path) = -3.250"
    assert len({len(l) for l in lines[:4]}) == 1                                                   # columns line up
    assert alignment_table(Alignment(np.full(4, -1, np.int32), -1e30, []), num_to_char).split("\n")[-1] == "no alignment"
    assert alignment_table(Alignment(np.zeros(1, np.int32), -0.5, [(9, 0, 1, 1.0)]), num_to_char).split("\n")[1].split()[1] == "?"
