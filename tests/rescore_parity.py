"""Shared by tests/test_rescore.py, tests/test_rescore_mutants.py and tests/test_rescore_gpu.py: the cases, the references, numpy restatements
of ishara_ctc_score_nbest (csrc/ctc_score.hip) and ishara_nbest_rescore (csrc/nbest_rescore.hip) with switchable mistakes, and the bounds.

Score cases (dict: name, logits float32 [B, T, C], blank, hyp_idx int32 [B, N, Th], hyp_len int32 [B, N], frame_len int32 [B] or None).  A
hypothesis is described as in tests/ctc_parity.py by (len, repeats): repeats are the positions i whose symbol equals symbol i - 1.  Symbol i is
lattice state 2 i + 1 and the kernel keeps state s in lane s % 64 of register s / 64, so symbols 32 k - 1 and 32 k sit on either side of a
register seam.  Dead slots hold the symbol 1000 everywhere, live rows 77 past their end in the cases marked poison; neither may be read.
  reference          ishara_amd.rescore.ctc_logp_reference (fp64 forward algorithm) on logits[b, :frame_len[b]], -inf for every slot the
                     contract gives -inf; expected_status() is the contract's status
  bound              |logp - ref| <= NLL_ATOL + NLL_RTOL |ref| of tests/ctc_parity.py, unchanged
  restate_score()    the recursion as the kernel arranges it, in fp64, with the mistakes of SCORE_MUTANTS

Rescore cases (dict: name, hyp_idx, hyp_len, logits (M arrays [B, T_m, C]: the models), nan_models (their logp is replaced by NaN: a model
that is not read), weights [M], lm, alpha, beta, inv_temp, C, blank).  The per-model logp fed to the kernel and to the reference are the same
float32 numbers: host_logps() here (the fp64 reference cast to float32), the device's own on the GPU.
  reference          ishara_amd.rescore.rescore_reference: out_score in every bit, order / perm / out_len / out_idx as integers
  posterior bound    p = e_i / sum_j e_j with e = expf(x), x = (s - s_max) * inv_temp.  Each e_j carries a relative error of at most
                     d_j = (2 |x_j| + K) * 2^-24 (mbr_parity: the two roundings on x, K for expf itself); a sequential sum of n <= 64
                     non-negative terms adds at most (n - 1) * 2^-24 relative and inherits at most max_j d_j; the division adds 2^-24.  To
                     first order |p - ref| <= ref * (d_i + max_j d_j + n * 2^-24); the second-order terms are below 1e-5 of that for
                     |x| <= 60, n <= 64 and are covered by the factor 1.001.  The cases keep x >= X_MIN = -60 (every e a normal float32).
  twin_rescore()     the kernel's arrangement (pairwise dedupe, rank by counting predecessors) in float32 with the mistakes of RESCORE_MUTANTS
"""
import functools

import numpy as np

import ctc_parity as CP
import mbr_parity as MP
from ishara_amd import mbr, rescore
from ishara_amd.ctc_lm import CharNGramLM

NLL_RTOL, NLL_ATOL = CP.NLL_RTOL, CP.NLL_ATOL
EPS, K, X_MIN = MP.EPS, MP.K, MP.X_MIN
DEAD_SYMBOL, PAST_END = 1000, 77
REGIMES = CP.REGIMES
SEAM_LENS = (0, 1, 31, 32, 33, 63, 64, 127, 128, 255)
SCORE_MUTANTS = ("skip_equal", "last_frame_dropped", "final_no_sm2", "frame_len_ignored")
RESCORE_MUTANTS = ("dedupe_ignores_length", "ties_to_higher", "weight_after_sum", "no_lm_eos", "beta_times_Th")


# ------------------------------------------------------------------------------------------------ hypotheses and logits
def make_hyp(g, n, rep, C, blank):
    """n symbols of [0, C) without blank; symbol i equals symbol i - 1 exactly at the positions in rep"""
    cls = np.array([c for c in range(C) if c != blank])
    h = []
    for i in range(n):
        if i > 0 and i in rep:
            h.append(h[-1])
        else:
            c = cls if i == 0 else cls[cls != h[-1]]
            h.append(int(c[g.integers(len(c))]))
    return h


def repeats_of(h):
    return sum(1 for i in range(1, len(h)) if h[i] == h[i - 1])


def make_logits(g, B, T, C, regime="n2", path=None):
    x = g.standard_normal((B, T, C))
    if regime == "n2":
        x *= 2
    elif regime == "n12":
        x *= 12
    elif regime == "flat":
        x *= 1e-3
    elif regime == "shift":
        x = 2 * x + 1000
    elif regime == "dead":
        x *= 2
        x[:, :, ::3] -= 80
    elif regime == "trained":
        for b in range(B):
            x[b, np.arange(T), path[b]] += 15
    return x.astype(np.float32)


def pack(clips, Th, poison=False):
    """clips: B lists of N entries (a symbol list, or None for a dead slot) -> hyp_idx int32 [B, N, Th], hyp_len int32 [B, N]"""
    B, N = len(clips), len(clips[0])
    idx = np.full((B, N, Th), PAST_END if poison else -1, np.int32)
    ln = np.zeros((B, N), np.int32)
    for b, hs in enumerate(clips):
        assert len(hs) == N
        for n, h in enumerate(hs):
            if h is None:
                idx[b, n], ln[b, n] = DEAD_SYMBOL, -1 - ((b + n) % 3)
            else:
                idx[b, n, :len(h)], ln[b, n] = h, len(h)
    return idx, ln


def score_case(name, clips, T, C, blank, Th, seed, regime="n2", frame_len=None, poison=False, nan_past_end=False):
    g = np.random.default_rng([7, seed])
    B = len(clips)
    path = None
    if regime == "trained":                                  # +15 along one alignment of each clip's first hypothesis
        path = [CP.path_of(np.array(hs[0] + [blank], np.int64), len(hs[0]), blank, T) for hs in clips]
    x = make_logits(g, B, T, C, regime, path)
    fl = None if frame_len is None else np.asarray(frame_len, np.int32)
    if nan_past_end:
        for b in range(B):
            if 1 <= fl[b] <= T:
                x[b, fl[b]:] = np.nan
            else:
                x[b] = np.nan                                # no frames: nothing of the clip is read
    idx, ln = pack(clips, Th, poison)
    c = dict(name=name, logits=x, blank=blank, hyp_idx=idx, hyp_len=ln, frame_len=fl, B=B, T=T, C=C, N=idx.shape[1], Th=Th)
    for k in ("logits", "hyp_idx", "hyp_len"):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def score_cases():
    out = []
    g = np.random.default_rng(4100)
    C, bl = 8, 7
    H = lambda n, rep=(): make_hyp(g, n, rep, C, bl)        # noqa: E731
    # the register seams: every length of SEAM_LENS, repeats on either side of a seam; Th differs from T
    seam = [[H(0), H(1), H(31), H(32), H(33), H(63), H(64), H(127)],
            [H(128), H(255), H(33, (32,)), H(64, (32, 40)), H(255, (32, 64, 96, 128, 160, 192, 224)), H(65, (64,)), H(129, (127, 128)), None]]
    out.append(score_case("seams", seam, 268, C, bl, 256, 1, poison=True))
    # one alignment only (T_b = len + repeats), and the same one frame short (no alignment), per clip through frame_len
    tight = [[H(32), H(31, (7,)), H(30, (3, 9)), H(33), H(31, (7, 20)), H(0)],
             [H(66), H(64, (32, 40)), H(65, (32,)), H(67), H(65, (32, 33)), H(1)],
             [H(1), H(2), H(1), H(1, ()), H(2, (1,)), H(0)]]
    out.append(score_case("tight", tight, 70, C, bl, 80, 2, frame_len=[32, 66, 1], poison=True))
    # ragged frame counts 0, 1, T, T + 1 with NaN in every row past a clip's end
    rag = [[H(0), H(1), H(3, (1,)), None]] * 4
    out.append(score_case("ragged", rag, 9, C, bl, 5, 3, frame_len=[0, 1, 9, 10], nan_past_end=True))
    rag2 = [[H(0), H(5), H(12, (4,)), H(33, (32,))], [H(2), H(6, (1, 2)), H(20), H(7)], [H(9), H(0), H(31), H(32)]]
    out.append(score_case("ragged-long", rag2, 45, C, bl, 45, 4, frame_len=[45, 23, 37], nan_past_end=True, poison=True))
    g64 = np.random.default_rng(4164)
    c64 = [[make_hyp(g64, n, rep, 64, 0) for n, rep in ((0, ()), (1, ()), (31, ()), (32, ()), (40, ()), (33, (32,)))]]
    out.append(score_case("C64-blank0", c64, 57, 64, 0, 57, 5))
    n64 = [[make_hyp(g, int(g.integers(0, 9)), (), C, bl) for _ in range(64)] for _ in range(2)]
    out.append(score_case("N64", n64, 16, C, bl, 16, 6))
    out.append(score_case("N1-T1", [[H(1)], [H(0)]], 1, C, bl, 1, 7))
    for r, regime in enumerate(REGIMES):                     # the logit regimes of ctc_parity.py
        hs = [[H(20, (5,)), H(0), H(1), H(33, (32,)), H(31), H(12)], [H(8), H(33), H(32, (31,)), H(2, (1,)), H(40), H(17)]]
        out.append(score_case(f"regime-{regime}", hs, 48, C, bl, 48, 10 + r, regime=regime))
    assert len({c["name"] for c in out}) == len(out)
    assert set(SEAM_LENS) <= {int(v) for v in out[0]["hyp_len"].ravel()}
    return tuple(out)


def bad_slot_case():
    """(case with a slot of every bad kind among good ones, the same case with the bad slots dead): status and isolation"""
    g = np.random.default_rng(4200)
    C, bl, Th = 8, 7, 12
    H = lambda n, rep=(): make_hyp(g, n, rep, C, bl)        # noqa: E731
    good = [[H(3), H(0), H(7, (2,)), H(5), H(9), H(2), H(1), H(4)], [H(6), H(2), H(0), H(10), H(3, (1, 2)), H(8), H(1), H(5)]]
    a = score_case("bad-slots", good, 14, C, bl, Th, 20, poison=True)
    idx, ln = a["hyp_idx"].copy(), a["hyp_len"].copy()
    want = np.zeros_like(ln)
    idx[0, 1], ln[0, 1], want[0, 1] = DEAD_SYMBOL, -2, rescore.STATUS_DEAD
    idx[0, 3, :5], want[0, 3] = [1, 2, 8, 3, 4], rescore.STATUS_SYMBOL                 # a symbol == C
    idx[0, 5, :2], want[0, 5] = [3, -1], rescore.STATUS_SYMBOL                         # a negative symbol
    idx[1, 0, :6], want[1, 0] = [1, 2, bl, 3, 4, 5], rescore.STATUS_SYMBOL             # the blank
    idx[1, 1, :2], want[1, 1] = [100000000, 1], rescore.STATUS_SYMBOL
    ln[1, 3], want[1, 3] = Th + 1, rescore.STATUS_LONG
    ln[1, 5], want[1, 5] = 4000, rescore.STATUS_LONG
    idx[1, 6], ln[1, 6], want[1, 6] = make_hyp(g, Th, (1, 2, 3), C, bl), Th, rescore.STATUS_NO_ALIGNMENT      # 12 + 3 > 14 frames
    bad = dict(a, hyp_idx=idx, hyp_len=ln, name="bad-slots")
    ln2 = np.where(want != 0, -1, ln).astype(np.int32)
    return bad, dict(a, hyp_idx=idx, hyp_len=ln2, name="bad-slots-removed"), want


def clip_frames(case, b):
    T = case["T"]
    tb = T if case["frame_len"] is None else int(case["frame_len"][b])
    return tb if 1 <= tb <= T else 0


def expected_status(case):
    B, N, Th, C, bl = case["B"], case["N"], case["Th"], case["C"], case["blank"]
    st = np.zeros((B, N), np.int32)
    for b in range(B):
        tb = clip_frames(case, b)
        for n in range(N):
            ln = int(case["hyp_len"][b, n])
            if ln < 0:
                st[b, n] = rescore.STATUS_DEAD
            elif ln > Th or ln > 255:
                st[b, n] = rescore.STATUS_LONG
            else:
                h = case["hyp_idx"][b, n, :ln].tolist()
                if any(v < 0 or v >= C or v == bl for v in h):
                    st[b, n] = rescore.STATUS_SYMBOL
                elif tb < 1 or tb < ln + repeats_of(h):
                    st[b, n] = rescore.STATUS_NO_ALIGNMENT
    return st


def score_reference_of(case):
    """fp64 [B, N]: ctc_logp_reference on the clip's own frames, -inf where the contract's status is not 0"""
    st = expected_status(case)
    ref = np.full(st.shape, -np.inf)
    for b in range(case["B"]):
        tb = clip_frames(case, b)
        for n in range(case["N"]):
            if st[b, n] == 0:
                h = case["hyp_idx"][b, n, :case["hyp_len"][b, n]]
                ref[b, n] = rescore.ctc_logp_reference(case["logits"][b, :tb].astype(np.float64), h, case["blank"])
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def score_reference(name):
    return score_reference_of(next(c for c in score_cases() if c["name"] == name))


def check_score(case, logp, status=None, ref=None):
    """(failures, worst err / bound) of logp [B, N] (and status) against the fp64 reference and the contract's status"""
    ref = score_reference(case["name"]) if ref is None else ref
    logp = np.asarray(logp, np.float64)
    want = expected_status(case)
    fails = []
    if status is not None and not np.array_equal(np.asarray(status), want):
        fails.append(f"{case['name']}: status {np.asarray(status).tolist()} != {want.tolist()}")
    dead = want != 0
    if not (np.isneginf(logp[dead])).all():
        fails.append(f"{case['name']}: a slot with a status is not -inf")
    with np.errstate(invalid="ignore"):
        r = np.abs(logp - ref) / (NLL_ATOL + NLL_RTOL * np.abs(ref))
    r = np.where(dead, 0.0, np.where(np.isfinite(logp), r, np.inf))
    ratio = float(r.max()) if r.size else 0.0
    if ratio > 1.0:
        fails.append(f"{case['name']}: logp err / bound {ratio:.3g} at {np.unravel_index(int(r.argmax()), r.shape)}")
    return fails, ratio


def restate_score(case, mutant=None):
    """ishara_ctc_score_nbest in fp64 as the kernel arranges it (extended sequence from the row, states s-1 / s-2, per-clip frame counts, the
    final sum of states S-1 and S-2, the status checks), with one of SCORE_MUTANTS switched on"""
    assert mutant is None or mutant in SCORE_MUTANTS, mutant
    B, N, T, Th, C, bl = case["B"], case["N"], case["T"], case["Th"], case["C"], case["blank"]
    out = np.full((B, N), -np.inf)
    st = np.zeros((B, N), np.int32)
    for b in range(B):
        tn = T if mutant == "frame_len_ignored" else clip_frames(case, b)
        x = case["logits"][b, :tn].astype(np.float64)
        m = x.max(axis=1, keepdims=True) if tn else x
        lp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))) if tn else x
        for n in range(N):
            ln = int(case["hyp_len"][b, n])
            if ln < 0:
                st[b, n] = 1
                continue
            if ln > Th or ln > 255:
                st[b, n] = 8
                continue
            h = case["hyp_idx"][b, n, :ln].astype(np.int64)
            if ((h < 0) | (h >= C) | (h == bl)).any():
                st[b, n] = 4
                continue
            if tn < 1 or tn < ln + repeats_of(h.tolist()):
                st[b, n] = 2
                continue
            S = 2 * ln + 1
            ext = np.full(S, bl, np.int64)
            ext[1::2] = h
            skip = np.zeros(S, bool)
            skip[2:] = (ext[2:] != bl) & ((ext[2:] != ext[:-2]) | (mutant == "skip_equal"))
            a = np.full(S, -np.inf)
            a[0] = lp[0, bl]
            if S > 1:
                a[1] = lp[0, ext[1]]
            last = tn - 1 if mutant == "last_frame_dropped" else tn
            with np.errstate(invalid="ignore"):
                for t in range(1, last):
                    a1 = np.concatenate([[-np.inf], a[:-1]])
                    a2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], a[:-2]]), -np.inf)
                    a = np.logaddexp(np.logaddexp(a, a1), a2) + lp[t, ext]
            v = a[S - 1]
            if S > 1 and mutant != "final_no_sm2":
                with np.errstate(invalid="ignore"):
                    v = np.logaddexp(v, a[S - 2])
            out[b, n] = v
            if not v > -1e29:
                out[b, n], st[b, n] = -np.inf, 2
    return out, st


# ------------------------------------------------------------------------------------------------ rescore cases
def _log_softmax_rows(g, C):
    t = g.standard_normal((C, C)) * 1.5
    return (t - np.log(np.exp(t).sum(axis=1, keepdims=True))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ngram4():
    g = np.random.default_rng(4300)
    phrases = [g.integers(0, 7, int(g.integers(1, 9))).tolist() for _ in range(60)]
    return CharNGramLM.fit(phrases, order=4, num_classes=8, blank=7)


def rescore_case(name, clips, Ts, seed, weights=None, lm=None, alpha=0.0, beta=0.0, inv_temp=None, nan_models=(), C=8, blank=7, Th=None):
    g = np.random.default_rng([9, seed])
    B = len(clips)
    Th = Th or max(max((len(h) for hs in clips for h in hs if h is not None), default=1), 1) + 2
    idx, ln = pack(clips, Th, poison=True)
    M = len(Ts)
    c = dict(name=name, hyp_idx=idx, hyp_len=ln, logits=tuple(make_logits(g, B, T, C) for T in Ts), nan_models=tuple(nan_models),
             weights=np.ones(M, np.float32) if weights is None else np.asarray(weights, np.float32), lm=lm, alpha=float(alpha), beta=float(beta),
             inv_temp=None if inv_temp is None else np.float32(inv_temp), C=C, blank=blank, B=B, N=idx.shape[1], Th=Th, M=M)
    return c


@functools.lru_cache(maxsize=None)
def rescore_cases():
    out = []
    g = np.random.default_rng(4400)
    C, bl = 8, 7
    H = lambda n, rep=(): make_hyp(g, n, rep, C, bl)        # noqa: E731
    base = [[H(3), H(4), H(3), H(0), H(5, (2,)), H(2), None, H(6)], [H(2), None, H(2), H(7), H(1), H(3), H(4, (1,)), H(5)]]
    dup01 = [list(hs) for hs in base]
    dup01[0][1] = list(dup01[0][0])                          # duplicates in slots 0 / 1
    dup01[1][7] = list(dup01[1][0])                          # and in slots 0 / N - 1
    dup01[1][4] = dup01[1][0][:1]                            # a proper prefix of slot 0: not a duplicate
    dup01[0][5] = dup01[0][4][:2]
    out.append(rescore_case("M1", dup01, (12,), 1))
    out.append(rescore_case("M3-weights-beta", dup01, (12, 20, 9), 2, weights=[0.5, 1.25, 0.25], beta=0.75, inv_temp=0.5))
    out.append(rescore_case("M8", base, (12, 20, 9, 16, 11, 30, 13, 10), 3, weights=[1, 0.5, 2, 0.125, 1, 3, 0.25, 1], inv_temp=0.1))
    out.append(rescore_case("zero-weight-over-nan", dup01, (12, 20, 9), 4, weights=[1.0, 0.0, 0.5], nan_models=(1,)))
    out.append(rescore_case("negative-and-nan-weights-not-read", base, (12, 20, 9), 5, weights=[-1.0, 1.0, np.nan], nan_models=(0, 2)))
    # exact ties: no model has a weight > 0, so s = beta * len and hypotheses of one length tie; the lower slot goes first
    out.append(rescore_case("exact-ties", base, (12,), 6, weights=[0.0], nan_models=(0,), beta=0.5))
    # model 1 has 4 frames: every hypothesis longer than that has no alignment there, logp_1 = -inf
    out.append(rescore_case("minus-inf-in-one-model", base, (12, 4), 7, weights=[1.0, 1.0], beta=0.25))
    out.append(rescore_case("all-dead", [[None] * 5, [H(2), None, H(1), None, None]], (12,), 8))
    out.append(rescore_case("bigram", dup01, (12, 15), 9, lm=_log_softmax_rows(g, C), alpha=0.6, beta=0.3, inv_temp=0.5))
    out.append(rescore_case("ngram4", dup01, (12, 15), 10, lm=ngram4(), alpha=0.4, beta=-0.2))
    out.append(rescore_case("ngram4-alpha0", base, (12,), 11, lm=ngram4(), alpha=0.0, beta=0.1))
    out.append(rescore_case("N1", [[H(3)], [None], [H(0)]], (12,), 12, lm=ngram4(), alpha=0.5))
    n64 = [[H(int(g.integers(0, 4))) if g.random() > 0.1 else None for _ in range(64)] for _ in range(2)]      # short strings: many duplicates
    out.append(rescore_case("N64", n64, (12, 9), 13, weights=[1.0, 0.5], lm=ngram4(), alpha=0.3, beta=0.5, inv_temp=0.25))
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def model_score_case(case, m):
    """model m of a rescore case as a score case"""
    x = case["logits"][m]
    return dict(name=f"{case['name']}-model{m}", logits=x, blank=case["blank"], hyp_idx=case["hyp_idx"], hyp_len=case["hyp_len"], frame_len=None,
                B=case["B"], T=x.shape[1], C=case["C"], N=case["N"], Th=case["Th"])


def host_logps(case):
    """float32 [M, B, N]: the fp64 reference under every model cast to float32, NaN for the models that must not be read"""
    out = np.stack([score_reference_of(model_score_case(case, m)).astype(np.float32) for m in range(case["M"])])
    for m in case["nan_models"]:
        out[m] = np.nan
    return out


def check_rescore(case, got, logps):
    """(failures, worst posterior err / bound) of a result (dict of out_idx [B, N, Th], out_len, out_score, posterior, perm) against
    rescore_reference fed the same float32 logps [M, B, N]"""
    B, N, Th = case["B"], case["N"], case["Th"]
    lists = mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])
    it = 1.0 if case["inv_temp"] is None else float(case["inv_temp"])
    fails, worst = [], 0.0
    for b in range(B):
        order, score, live, post = rescore.rescore_reference(lists[b], logps[:, b], case["weights"], case["lm"], case["alpha"], case["beta"], it,
                                                             case["blank"])
        if not np.array_equal(np.asarray(got["perm"][b], np.int64), order):
            fails.append(f"clip {b}: perm {np.asarray(got['perm'][b]).tolist()} != {order.tolist()}")
            continue
        if not np.array_equal(np.asarray(got["out_score"][b], np.float32).view(np.uint32), score.view(np.uint32)):
            fails.append(f"clip {b}: out_score {np.asarray(got['out_score'][b]).tolist()} != {score.tolist()}")
        want_len = np.array([len(lists[b][k]) if lv else -1 for k, lv in zip(order, live)], np.int64)
        want_idx = np.full((N, Th), -1, np.int64)
        for r, (k, lv) in enumerate(zip(order, live)):
            if lv:
                want_idx[r, :want_len[r]] = lists[b][k]
        if not np.array_equal(np.asarray(got["out_len"][b]), want_len) or not np.array_equal(np.asarray(got["out_idx"][b]), want_idx):
            fails.append(f"clip {b}: out_idx / out_len are not the reference's rows in the reference's order")
        p = np.asarray(got["posterior"][b], np.float64)
        fin = live & np.isfinite(score)
        if (p[~fin] != 0).any() or np.signbit(np.asarray(got["posterior"][b])[~fin]).any():
            fails.append(f"clip {b}: a slot without a finite score has a posterior")
        if fin.any():
            s64 = score.astype(np.float64)
            x = (s64[fin] - s64[fin].max()) * it
            assert x.min() >= X_MIN, (case["name"], x.min())
            d = (2.0 * np.abs(x) + K) * EPS
            bound = post[fin] * (d + d.max() + int(fin.sum()) * EPS) * 1.001
            r = np.abs(p[fin] - post[fin]) / bound
            r = np.where(np.isfinite(p[fin]), r, np.inf)
            worst = max(worst, float(r.max()))
            if abs(p[fin].sum() - 1.0) > 64 * 2 * EPS + float(bound.sum()):
                fails.append(f"clip {b}: the posterior sums to {p[fin].sum()!r}")
    if worst > 1.0:
        fails.append(f"posterior err / bound {worst:.3g}")
    return fails, worst


def twin_rescore(case, logps, mutant=None):
    """ishara_nbest_rescore in numpy as the kernel arranges it: pairwise dedupe, float32 score with one rounding per operation, rank =
    the number of slots that precede, float32 posterior summed in output order; `mutant`: one of RESCORE_MUTANTS"""
    assert mutant is None or mutant in RESCORE_MUTANTS, mutant
    f32 = np.float32
    B, N, Th, M = case["B"], case["N"], case["Th"], case["M"]
    aut = rescore._lm_host(case["lm"], case["blank"])
    w = case["weights"]
    it = f32(1.0) if case["inv_temp"] is None else f32(case["inv_temp"])
    out = dict(out_idx=np.full((B, N, Th), -1, np.int32), out_len=np.full((B, N), -1, np.int32), out_score=np.full((B, N), -np.inf, f32),
               posterior=np.zeros((B, N), f32), perm=np.zeros((B, N), np.int32))
    with np.errstate(all="ignore"):
        for b in range(B):
            ln = np.minimum(case["hyp_len"][b].astype(np.int64), Th)
            ln = np.where(ln < 0, -1, ln)
            hyp = case["hyp_idx"][b]
            dup = np.zeros(N, bool)
            for i in range(N):
                for j in range(i + 1, N):
                    if ln[i] < 0 or ln[j] < 0:
                        continue
                    if mutant == "dedupe_ignores_length":
                        k = min(ln[i], ln[j])
                        same = np.array_equal(hyp[i, :k], hyp[j, :k])
                    else:
                        same = ln[i] == ln[j] and np.array_equal(hyp[i, :ln[i]], hyp[j, :ln[j]])
                    if same:
                        dup[j] = True
            live = (ln >= 0) & ~dup
            s = np.zeros(N, f32)
            for n in np.nonzero(live)[0]:
                v = f32(0.0)
                if mutant == "weight_after_sum":             # the sum of the participating models times the last weight
                    wl = f32(1.0)
                    for m in range(M):
                        if w[m] > 0:
                            v, wl = f32(v + logps[m, b, n]), w[m]
                    v = f32(wl * v)
                else:
                    for m in range(M):
                        if w[m] > 0:
                            v = f32(v + f32(w[m] * logps[m, b, n]))
                if aut is not None:
                    l, state = f32(0.0), aut.start
                    for c in hyp[n, :ln[n]]:
                        l = f32(l + aut.logp[state, c])
                        state = int(aut.next[state, c])
                    if mutant != "no_lm_eos":
                        l = f32(l + aut.logp[state, case["blank"]])
                    v = f32(v + f32(f32(case["alpha"]) * l))
                v = f32(v + f32(f32(case["beta"]) * f32(Th if mutant == "beta_times_Th" else ln[n])))
                s[n] = v
            cls = np.where(~live, 2, np.where(np.isnan(s), 1, 0))
            rank = np.zeros(N, np.int64)
            for i in range(N):
                for j in range(N):
                    if j == i:
                        continue
                    lower = j > i if mutant == "ties_to_higher" else j < i
                    if cls[j] < cls[i] or (cls[j] == cls[i] and ((s[j] > s[i] or (s[j] == s[i] and lower)) if cls[i] == 0 else j < i)):
                        rank[i] += 1
            perm = np.zeros(N, np.int64)
            perm[rank] = np.arange(N)
            so, lo = s[perm], np.where(live[perm], ln[perm], -1)
            fin = (lo >= 0) & (np.abs(so) < np.inf)
            e = np.zeros(N, f32)
            if fin.any():
                e[fin] = np.exp(((so[fin] - so[fin].max()).astype(f32) * it).astype(f32)).astype(f32)
            tot = f32(0.0)
            for r in range(N):
                tot = f32(tot + e[r])
            out["perm"][b] = perm
            out["out_len"][b] = lo
            out["out_score"][b] = np.where(lo >= 0, so, f32(-np.inf))
            out["posterior"][b] = np.where(fin & (tot > 0), e / (tot if tot > 0 else f32(1.0)), f32(0.0)).astype(f32)
            for r in range(N):
                if lo[r] >= 0:
                    out["out_idx"][b, r, :lo[r]] = hyp[perm[r], :lo[r]]
    return out
