"""Shared by tests/test_rescore_sweep.py, tests/test_rescore_sweep_mutants.py and tests/test_rescore_sweep_gpu.py: the cases of
ishara_rescore_sweep (csrc/rescore_sweep.hip), the reference glue and a numpy restatement of the kernel with switchable mistakes.

A case is a dict: name, hyp_idx int32 [B, N, Th], hyp_len int32 [B, N] (tests/rescore_parity.py's pack: dead rows hold 1000, live rows 77
past their end), logps float32 [M, B, N] (the numbers both the device and the reference are fed; the sweep takes scores, not logits, so Th
is a row stride that belongs to no model's T; the GPU test also runs the 80-wide `lengths` rows on scores the device took at T = 96), targets int32 [B, L] padded with 59, grid float32 [G, M + 2], lm (None, a [C, C] table or a
CharNGramLM), C, blank, and `coverage`: the case counts as a random case of the coverage condition.  Every case is run with fallback 0 and 1.
  reference          ishara_amd.rescore.rescore_sweep_reference per clip (rescore_reference + evaluation.levenshtein +
                     tflite_batch.apply_fallback): best, dist, tlen, hyp_dist as integers; lm_walk() is the float32 walk lm_score must
                     equal bit for bit
  twin_sweep()       the kernel's arrangement: pairwise dedupe, one float32 walk per slot, the distance by the 64-bit Myers / Hyyro word
                     with the target as the pattern (Python integers masked to 64 bits), max-then-lowest-set-bit selection; `mutant`: one
                     of SWEEP_MUTANTS
G takes 1, 2, 63, 64, 65 and SWEEP_ROW_TILE - 1, SWEEP_ROW_TILE, SWEEP_ROW_TILE + 1 (the launcher's rows per workgroup, 256)."""
import functools

import numpy as np

import rescore_parity as RP
from ishara_amd import mbr, rescore
from ishara_amd.ctc_lm import CharNGramLM
from ishara_amd.tflite_model import FALLBACK_PHRASE

PAD = 59
TILE = rescore.SWEEP_ROW_TILE
G_EDGES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1)
SWEEP_MUTANTS = ("ties_to_higher", "merged_wins", "no_fallback", "fallback_at_3", "nonpositive_weight_read", "grid_stride_M1", "no_lm_eos",
                 "neighbour_target", "nan_outranks_minus_inf", "beta_times_Th")
F32 = np.float32


# ------------------------------------------------------------------------------------------------ building blocks
@functools.lru_cache(maxsize=None)
def ngram4_60():
    g = np.random.default_rng(5300)
    phrases = [g.integers(0, 59, int(g.integers(2, 20))).tolist() for _ in range(80)]
    return CharNGramLM.fit(phrases, order=4, num_classes=60, blank=59)


def bigram(seed, C=60, minus_inf=()):
    g = np.random.default_rng([53, seed])
    t = g.standard_normal((C, C)) * 1.5
    t = (t - np.log(np.exp(t).sum(axis=1, keepdims=True))).astype(F32)
    for r, c in minus_inf:
        t[r, c] = -np.inf
    return t


def pad_targets(tgts, L):
    out = np.full((len(tgts), L), PAD, np.int32)
    for b, t in enumerate(tgts):
        out[b, :len(t)] = t
    return out


def make_case(name, clips, logps, tgts, grid, lm=None, C=60, blank=None, Th=None, L=None, coverage=False):
    B, N = len(clips), len(clips[0])
    Th = Th or max(max((len(h) for hs in clips for h in hs if h is not None), default=1), 1) + 3
    idx, ln = RP.pack(clips, Th, poison=True)
    logps = np.asarray(logps, F32)
    grid = np.asarray(grid, F32)
    assert logps.ndim == 3 and logps.shape[1:] == (B, N) and grid.ndim == 2 and grid.shape[1] == logps.shape[0] + 2, name
    L = L or max(max(len(t) for t in tgts), 1)
    c = dict(name=name, hyp_idx=idx, hyp_len=ln, logps=logps, targets=pad_targets(tgts, L), grid=grid, lm=lm, C=C, blank=C - 1 if blank is None else blank,
             B=B, N=N, Th=Th, M=logps.shape[0], G=grid.shape[0], L=L, coverage=coverage)
    for k in ("hyp_idx", "hyp_len", "logps", "targets", "grid"):
        c[k].setflags(write=False)
    return c


def noisy(g, tgt, C=59):
    """a hypothesis near the target: each symbol kept, dropped, replaced or followed by an extra one"""
    h = []
    for v in tgt:
        r = g.random()
        if r < 0.12:
            continue
        h.append(int(g.integers(0, C)) if r < 0.3 else int(v))
        if g.random() < 0.1:
            h.append(int(g.integers(0, C)))
    return h


def random_grid(g, G, M):
    grid = np.concatenate([g.uniform(0.0, 2.0, (G, M)), g.uniform(0.0, 1.5, (G, 1)), g.uniform(-3.0, 3.0, (G, 1))], axis=1).astype(F32)
    grid[:, :M][g.random((G, M)) < 0.15] = 0.0                # models switched off here and there
    return grid


def random_case(name, seed, B, N, M, G, lm=None, dead=0.1):
    g = np.random.default_rng([57, seed])
    tgts = [g.integers(0, 59, int(g.integers(4, 31))).tolist() for _ in range(B)]
    clips = []
    for b in range(B):
        hs = [noisy(g, tgts[b]) if g.random() > dead else None for _ in range(N)]
        if N > 2 and hs[0] is not None:
            hs[N - 1] = list(hs[0])                          # a duplicate of slot 0 in the last slot
        clips.append(hs)
    # scores that disagree between the models, so that the rows of the grid pick different slots
    logps = (-g.uniform(5.0, 20.0, (M, B, N))).astype(F32)
    return make_case(name, clips, logps, tgts, random_grid(g, G, M), lm, coverage=N >= 5 and G >= 63)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    g = np.random.default_rng(5400)
    H = lambda n: g.integers(0, 59, n).tolist()              # noqa: E731
    big, ng = bigram(1), ngram4_60()
    # ---- the random cases: N x M x G x LM kind
    out.append(random_case("r-N1-M1-G1", 1, 2, 1, 1, 1, dead=0.0))
    out.append(random_case("r-N5-M3-G2-bigram", 2, 3, 5, 3, 2, big))
    out.append(random_case("r-N64-M8-G63-ngram4", 3, 2, 64, 8, 63, ng))
    out.append(random_case("r-N5-M1-G64", 4, 3, 5, 1, 64))
    out.append(random_case("r-N64-M3-G65-bigram", 5, 2, 64, 3, 65, big))
    out.append(random_case(f"r-N5-M8-G{TILE - 1}", 6, 3, 5, 8, TILE - 1))
    out.append(random_case(f"r-N64-M1-G{TILE}-ngram4", 7, 2, 64, 1, TILE, ng))
    out.append(random_case(f"r-N5-M3-G{TILE + 1}", 8, 3, 5, 3, TILE + 1))
    # ---- lengths: a 64-symbol target against hypotheses of 64 and 70 (bit 63 of the word), a 1-symbol target, hypotheses of 0, 2, 3
    # (the fallback edge on both sides), three different targets in one batch
    t64 = H(64)
    h64 = list(t64)
    h64[63] = (h64[63] + 1) % 59                             # differs in the last symbol only
    h70 = t64[:40] + H(6) + t64[40:]
    t1 = [5]
    t10 = H(10)
    clips = [[h64, h70, [], t64[:2], t64[:3]], [[], [5, 7], [5, 7, 9], [5], H(5)], [t10[:3], t10[:2], list(t10), [], H(12)]]
    lg = -g.uniform(1.0, 30.0, (1, 3, 5))
    grid = np.array([[1, 0, 0], [1, 0, 2.0], [1, 0, -2.0], [0.5, 0, 0.4], [2, 0, -0.37], [1, 0, 9.0], [1, 0, -9.0]], F32)
    out.append(make_case("lengths", clips, lg, [t64, t1, t10], grid, Th=80, L=64))
    # ---- ties: slots 1 and 3 hold different strings of one length with equal scores: a tie at every row
    tie = [[H(6), H(7), H(9), H(7), H(4)], [H(5), H(8), H(3), H(8), H(8)]]
    lg = -g.uniform(20.0, 30.0, (2, 2, 5))
    lg[:, :, 1] = lg[:, :, 3] = -3.0
    out.append(make_case("tie-every-row", tie, lg, [H(7), H(8)], random_grid(np.random.default_rng(1), 7, 2) + F32([0.25, 0.25, 0, 0])))
    # a tie at one row only: the row whose weights are all 0, s = beta * len, and slots 1 / 3 / 4 of clip 1 share the longest length
    grid = np.array([[1.0, 0.5, 0, 0.1], [0, 0, 0, 0.5], [0.3, 1.0, 0, -0.2]], F32)
    lg = -g.uniform(5.0, 30.0, (2, 2, 5))
    out.append(make_case("tie-one-row", tie, lg, [H(7), H(8)], grid))
    # ---- weights that are not > 0 over arrays of NaN: models 0..2 are never read at rows 0..2; row 3 reads model 0: every score NaN
    lg = -g.uniform(5.0, 30.0, (4, 2, 5))
    lg[:3] = np.nan
    grid = np.array([[0, -1, np.nan, 1.0, 0, 0.2], [-0.0, -2, np.nan, 0.5, 0, -0.3], [np.nan, 0, -1, 2.0, 0, 1.5], [1.0, 0, 0, 1.0, 0, 0.1]], F32)
    out.append(make_case("nonpositive-weights-over-nan", tie, lg, [H(7), H(8)], grid))
    # ---- -inf in one model, a NaN slot, a clip whose numbers are all -inf, a symbol outside [0, C) under an LM
    rows = [[H(6), H(7), H(9), H(5), H(4)], [H(5), H(8), H(3), H(6), H(7)], [H(4), H(2), H(6), H(3), H(5)]]
    rows[2][3] = [3, 1000, 4]                                # under the LM: score -inf; to the distance: a symbol like any other
    lg = -g.uniform(5.0, 30.0, (2, 3, 5))
    lg[1, 0, [0, 2]] = -np.inf
    lg[0, 0, 1] = np.nan                                     # a NaN slot among numbers
    lg[1, 1, :] = -np.inf                                    # clip 1: every number is -inf: the lowest live slot
    lg[0, 1, 2] = np.nan                                     # and a NaN slot that must not outrank them
    grid = np.array([[1, 1, 0.3, 0.2], [1, 0, 0.5, -0.1], [0, 1, 0.2, 0.4], [0.5, 2, 0, 0], [1, 1, 1.0, 1.0]], F32)
    out.append(make_case("minus-inf-and-nan-slots", rows, lg, [H(6), H(6), H(5)], grid, big))
    clip1 = [list(h) for h in rows[1]]
    lg2 = lg.copy()
    lg2[0, 1, 0], lg2[1, 1, 0] = np.nan, 0.0                 # slot 0 a NaN, the rest -inf: slot 1 (-inf) tops the list
    out.append(make_case("nan-slot-0-never-tops-minus-inf", [rows[0], clip1, rows[2]], lg2, [H(6), H(6), H(5)], grid[:, [0, 1, 2, 3]] * F32([1, 1, 0, 1])))
    # ---- liveness: every slot dead; one live slot that is not slot 0
    dead = [[None] * 5, [None, None, None, H(6), None], [None, H(2), None, None, None]]
    lg = -g.uniform(5.0, 30.0, (1, 3, 5))
    out.append(make_case("all-dead-and-one-live", dead, lg, [H(6), H(6), H(5)], np.array([[1, 0, 0], [0.5, 0, 0.7], [0, 0, -1]], F32)))
    # ---- duplicates in slots 0 / 1 and 0 / N - 1: the later copy has the larger score
    dup = [[H(6), None, H(7), H(5), H(4)], [H(5), H(8), H(6), H(7), None]]
    dup[0][1] = list(dup[0][0])
    dup[1][4] = list(dup[1][0])
    dup[1][2] = dup[1][0][:3]                                # a proper prefix: not a duplicate
    lg = -g.uniform(20.0, 30.0, (2, 2, 5))
    lg[:, 0, 1] = -1.0
    lg[:, 1, 4] = -1.0
    lg[0, :, 0] = -15.0                                      # slot 0 tops the list at the rows that read model 0 only
    for kind, lm in (("none", None), ("bigram", big), ("ngram4", ng)):
        out.append(make_case(f"duplicates-{kind}", dup, lg, [dup[0][2], dup[1][3]], random_grid(np.random.default_rng(2), 7, 2), lm))
    # ---- alpha = 0 over a hypothesis the LM gives -inf: 0 * -inf is NaN and the slot ranks as one
    binf = bigram(3, minus_inf=((4, 9), (9, 4)))
    rows = [[[1, 4, 9, 2, 7], [1, 4, 8, 2], [3, 9, 4], [2, 2, 2, 6]], [[4, 9], [9, 4, 9], [6, 6, 6], [1, 2, 3]]]
    lg = -g.uniform(5.0, 30.0, (1, 2, 4))
    lg[0, :, 0] = -1.0                                       # the -inf hypotheses have the best model score
    grid = np.array([[1, 0, 0.2], [1, 0.5, 0.2], [1, 0, -0.4], [0, 0, 1.0], [1, -0.5, 0]], F32)
    out.append(make_case("alpha0-lm-minus-inf", rows, lg, [[1, 4, 9, 2], [6, 6, 6]], grid, binf))
    # ---- C = 3: small enough for the brute force of the CPU test (one symbol apart from blank and one more)
    g3 = np.random.default_rng(5403)
    rows = [[g3.integers(0, 2, int(g3.integers(0, 7))).tolist() if g3.random() > 0.15 else None for _ in range(6)] for _ in range(3)]
    lg = -g3.uniform(1.0, 12.0, (2, 3, 6))
    tg = [g3.integers(0, 2, n).tolist() for n in (5, 1, 3)]
    out.append(make_case("C3", rows, lg, tg, random_grid(g3, 9, 2), bigram(4, C=3), C=3))
    assert len({c["name"] for c in out}) == len(out)
    assert {c["G"] for c in out} >= set(G_EDGES) and {c["N"] for c in out} >= {1, 5, 64} and {c["M"] for c in out} >= {1, 3, 8}
    return tuple(out)


# ------------------------------------------------------------------------------------------------ the reference
def lm_walk(case):
    """float32 [B, N]: l of every slot that survives the merge (-inf for a symbol outside [0, C)), +0 elsewhere and without an LM"""
    aut = rescore._lm_host(case["lm"], case["blank"])
    B, N = case["B"], case["N"]
    out = np.zeros((B, N), F32)
    if aut is None:
        return out
    lists = mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])
    with np.errstate(all="ignore"):
        for b in range(B):
            seen = set()
            for n, h in enumerate(lists[b]):
                if h is None or tuple(h) in seen:
                    continue
                seen.add(tuple(h))
                if any(c < 0 or c >= case["C"] for c in h):
                    out[b, n] = -np.inf
                    continue
                l, state = F32(0.0), aut.start
                for c in h:
                    l = F32(l + aut.logp[state, c])
                    state = int(aut.next[state, c])
                out[b, n] = F32(l + aut.logp[state, case["blank"]])
    return out


@functools.lru_cache(maxsize=None)
def reference(name, fallback):
    """dict of best [G, B], dist [G, B], tlen [B], hyp_dist [B, N] (int64) by rescore_sweep_reference, clip by clip; computed once"""
    case = next(c for c in cases() if c["name"] == name)
    lists = mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])
    B, N, G = case["B"], case["N"], case["G"]
    ref = dict(best=np.zeros((G, B), np.int64), dist=np.zeros((G, B), np.int64), tlen=np.zeros(B, np.int64), hyp_dist=np.zeros((B, N), np.int64))
    for b in range(B):
        best, dist, tlen, hd = rescore.rescore_sweep_reference(lists[b], case["logps"][:, b], case["targets"][b], case["grid"], case["lm"], case["blank"],
                                                               bool(fallback))
        ref["best"][:, b], ref["dist"][:, b], ref["tlen"][b], ref["hyp_dist"][b] = best, dist, tlen, hd
    for v in ref.values():
        v.setflags(write=False)
    return ref


def compare(case, fallback, got):
    """the keys of got (best, dist, tlen, hyp_dist) that differ from the reference"""
    ref = reference(case["name"], int(fallback))
    return [k for k in ("best", "dist", "tlen", "hyp_dist") if k in got and not np.array_equal(np.asarray(got[k], np.int64), ref[k])]


# ------------------------------------------------------------------------------------------------ the kernel, restated
def myers(tgt, text):
    """Levenshtein distance by the 64-bit word with `tgt` (<= 64 symbols) as the pattern"""
    m, W = len(tgt), (1 << 64) - 1
    if m == 0:
        return len(text)
    pv, mv, top, score = W, 0, 1 << (m - 1), m
    for c in text:
        eq = sum(1 << j for j, t in enumerate(tgt) if t == c)
        xv = eq | mv
        xh = ((((eq & pv) + pv) & W) ^ pv) | eq
        ph = (mv | ~(xh | pv)) & W
        mh = pv & xh
        score += 1 if ph & top else 0
        score -= 1 if mh & top else 0
        ph = ((ph << 1) | 1) & W
        mh = (mh << 1) & W
        pv = (mh | ~(xv | ph)) & W
        mv = ph & xv
    return score


def twin_sweep(case, fallback, mutant=None):
    assert mutant is None or mutant in SWEEP_MUTANTS, mutant
    B, N, Th, M, G = case["B"], case["N"], case["Th"], case["M"], case["G"]
    aut = rescore._lm_host(case["lm"], case["blank"])
    flat = case["grid"].ravel()
    stride = M + 1 if mutant == "grid_stride_M1" else M + 2
    fb_on = bool(fallback) and mutant != "no_fallback"
    fb_len = 4 if mutant == "fallback_at_3" else 3
    phrase = [int(v) for v in FALLBACK_PHRASE]
    out = dict(best=np.zeros((G, B), np.int64), dist=np.zeros((G, B), np.int64), tlen=np.zeros(B, np.int64), hyp_dist=np.full((B, N), -1, np.int64))
    with np.errstate(all="ignore"):
        for b in range(B):
            tb = (b + 1) % B if mutant == "neighbour_target" else b
            tgt = rescore.target_symbols(case["targets"][tb])
            out["tlen"][b] = len(rescore.target_symbols(case["targets"][b]))
            ln = np.where(case["hyp_len"][b] < 0, -1, np.minimum(case["hyp_len"][b], Th)).astype(np.int64)
            hyp = case["hyp_idx"][b]
            dup = np.zeros(N, bool)
            for i in range(N):
                for j in range(i + 1, N):
                    if ln[i] >= 0 and ln[i] == ln[j] and np.array_equal(hyp[i, :ln[i]], hyp[j, :ln[j]]):
                        dup[j] = True
            live = (ln >= 0) & ~dup
            l, bad, hd = np.zeros(N, F32), np.zeros(N, bool), np.full(N, -1, np.int64)
            for n in np.nonzero(ln >= 0)[0]:
                h = hyp[n, :ln[n]].tolist()
                if aut is not None:
                    if any(c < 0 or c >= case["C"] for c in h):
                        bad[n] = True
                    else:
                        v, state = F32(0.0), aut.start
                        for c in h:
                            v = F32(v + aut.logp[state, c])
                            state = int(aut.next[state, c])
                        l[n] = v if mutant == "no_lm_eos" else F32(v + aut.logp[state, case["blank"]])
                hd[n] = myers(tgt, phrase if fb_on and ln[n] < fb_len else h)
            out["hyp_dist"][b] = np.where(live, hd, -1)
            none_d = myers(tgt, phrase) if fb_on else len(tgt)
            can_win = (ln >= 0) if mutant == "merged_wins" else live
            for gi in range(G):
                p = flat[gi * stride: gi * stride + M + 2]
                if p.shape[0] < M + 2:
                    p = np.concatenate([p, np.zeros(M + 2 - p.shape[0], F32)])
                s = np.zeros(N, F32)
                for n in range(N):
                    v = F32(0.0)
                    for m in range(M):
                        if p[m] > 0 or (mutant == "nonpositive_weight_read" and p[m] == p[m]):
                            v = F32(v + F32(p[m] * case["logps"][m, b, n]))
                    if aut is not None:
                        v = F32(-np.inf) if bad[n] else F32(v + F32(p[M] * l[n]))
                    s[n] = F32(v + F32(p[M + 1] * F32(Th if mutant == "beta_times_Th" else ln[n])))
                if mutant == "nan_outranks_minus_inf":
                    s = np.where(np.isnan(s), F32(-3e38), s)
                num = can_win & ~np.isnan(s)
                if num.any():
                    top = np.nonzero(num & (s == s[num].max()))[0]
                    win = int(top[-1] if mutant == "ties_to_higher" else top[0])
                else:
                    win = int(np.nonzero(can_win)[0][0]) if can_win.any() else -1
                out["best"][gi, b] = win
                out["dist"][gi, b] = hd[win] if win >= 0 else none_d
    return out


def coverage(case):
    """(the fraction of clips with three or more distinct winning slots across the grid, whether some row picks a slot other than 0)"""
    best = reference(case["name"], 1)["best"]
    many = np.mean([len(set(best[:, b].tolist()) - {-1}) >= 3 for b in range(case["B"])])
    return float(many), bool((best != 0).any())
