"""Shared by tests/test_mbr.py, tests/test_mbr_mutants.py and tests/test_mbr_gpu.py: the case table of ishara_mbr_select, the glue to
ishara_amd.mbr.mbr_reference, a numpy twin of the kernel's arithmetic (bit-vector edit distance, float32 votes and risk) with switchable
mistakes, and the comparison both the twin and the device go through.

What `check` asks of a result (dict of out_idx [B, T], out_len [B], best [B], risk [B, N], w_out [B, N], dist [B, N, N], status [B]):
  1. dist, best, out_idx, out_len and status equal mbr_reference's exactly, the reference run with votes = the result's own w_out;
  2. risk equals, in every bit (NaN rows included), the float32 recomputation from that w_out in the contract's order, so best is the argmin
     of exactly the numbers the device had: nothing is left out, there is no margin and no excluded share;
  3. w_out against the fp64 votes: explicit weights exactly; exp votes within ref * (2 |x| + K) * 2^-24, x = (s - s_max) * inv_temp.  The
     two fp32 roundings on x (the subtraction, the multiplication) move it by at most |x| * 2^-23 = 2 |x| * 2^-24, which is the relative
     error they leave on exp(x); K covers expf itself.  K is not fitted to the device: K_HOST is the worst (err / (ref * 2^-24) - 2 |x|) of
     the unmutated float32 twin (numpy's float32 exp) over the whole table, measured on the CPU (`measure_k_host`, printed by
     tests/test_mbr_mutants.py), and K = 4 * K_HOST, which leaves room for a device expf that is an ulp or two worse than numpy's.  The
     cases keep x >= -60, so every vote is a normal float32.
`check` returns (failures, ratio): the list of violated items and the worst err / bound of item 3 (inf for a NaN).

A case is a dict: name, B, N, T, C, mode, hyp_idx int32 [B, N, T], hyp_len int32 [B, N], hyp_score float32 [B, N] or None, weights float32
[B, N] or None, inv_temp (a float32 or None).  Dead slots (hyp_len < 0) hold the symbol 1000 everywhere and a finite score above every live
one; rows of live slots hold 77 past their end in the cases marked `poison`: neither may be read."""
import functools

import numpy as np

from ishara_amd import mbr

EPS = 2.0 ** -24
K_HOST = 1.25         # measured: measure_k_host() gives 1.204 over the table (numpy's float32 exp, within 0.6 ulp of 2^-23); see DESIGN.md
K = 4 * K_HOST
X_MIN = -60.0
LENS_ALL = (0, 1, 2, 31, 32, 33, 63, 64)
NS = (1, 2, 3, 31, 32, 33, 63, 64)
TS = (1, 5, 64, 65, 384)
CS = (2, 59, 60, 64)
MUTANTS = ("first_row_zero", "carry_dropped", "top_bit_63", "shift_by_64", "norm_by_candidate", "dead_slot_votes", "ties_to_higher", "fma",
           "reverse_sum", "unshifted_scores", "no_status_long")
DEAD_SYMBOL, PAST_END = 1000, 77


def _hyps(g, N, T, C, lens, base_len=64):
    """N hypotheses: one random base string, each copy with up to three random edits, cut or extended to its length"""
    base = g.integers(0, C, base_len).tolist()
    out = []
    for n in range(N):
        h = list(base)
        for _ in range(int(g.integers(0, 4))):
            p, kind = int(g.integers(0, len(h) + 1)), int(g.integers(0, 3))
            if kind == 0 and p < len(h):
                h[p] = int(g.integers(0, C))
            elif kind == 1 and p < len(h):
                del h[p]
            else:
                h.insert(p, int(g.integers(0, C)))
        want = lens[n]
        h = h[:want] + g.integers(0, C, max(want - len(h), 0)).tolist()
        out.append(h)
    return out


def build(name, clips, T, C, mode, scores=None, weights=None, inv_temp=None, poison=False, raw_len=None):
    """clips: B lists of N entries (a symbol list, or None for a dead slot).  scores / weights: [B, N] arrays.  raw_len: hyp_len to store in
    place of the true lengths (the clamp to T)."""
    B, N = len(clips), len(clips[0])
    idx = np.full((B, N, T), PAST_END if poison else -1, np.int32)
    ln = np.zeros((B, N), np.int32)
    for b, hs in enumerate(clips):
        for n, h in enumerate(hs):
            if h is None:
                idx[b, n], ln[b, n] = DEAD_SYMBOL, -1 - ((b + n) % 3)
            else:
                idx[b, n, :len(h)], ln[b, n] = h, len(h)
    if raw_len is not None:
        ln = np.asarray(raw_len, np.int32)
    c = dict(name=name, B=B, N=N, T=T, C=C, mode=mode, hyp_idx=idx, hyp_len=ln, hyp_score=None if scores is None else np.asarray(scores, np.float32),
             weights=None if weights is None else np.asarray(weights, np.float32), inv_temp=None if inv_temp is None else np.float32(inv_temp))
    for k in ("hyp_idx", "hyp_len", "hyp_score", "weights"):
        if c[k] is not None:
            c[k].setflags(write=False)
    return c


def _scores(g, clips, spread=6.0):
    """ranked natural-log scores per clip (descending over the live slots), dead slots above all of them"""
    out = np.zeros((len(clips), len(clips[0])), np.float32)
    for b, hs in enumerate(clips):
        live = [n for n, h in enumerate(hs) if h is not None]
        s = -np.sort(g.random(len(live)) * spread) - 40.0 * g.random()
        out[b, live] = s
        out[b, [n for n, h in enumerate(hs) if h is None]] = 3.5
    return out


def _random_case(i, N, B, T, C, mode, votes, inv_temp, dead=0.0, poison=False):
    g = np.random.default_rng(2100 + i)
    cap = min(T, 64)
    pool = [v for v in LENS_ALL if v <= cap] or [0, cap]
    if cap not in pool:
        pool.append(cap)
    clips = []
    for b in range(B):
        lens = [pool[(n + b + i) % len(pool)] for n in range(N)]
        hs = _hyps(g, N, T, C, lens)
        clips.append([None if g.random() < dead else h for h in hs])
    sc = _scores(g, clips) if votes == "scores" else None
    w = (g.random((B, N)) * 2).astype(np.float32) if votes == "weights" else None
    return build(f"{i:02d}-N{N}-B{B}-T{T}-C{C}-mode{mode}-{votes}" + ("-dead" if dead else "") + ("-poison" if poison else ""), clips, T, C, mode, sc, w,
                 inv_temp, poison)


@functools.lru_cache(maxsize=None)
def cases():
    out, i = [], 0
    for k, N in enumerate(NS):                               # every N in both modes; T, C, B, the votes and the temperature rotate
        for mode in (0, 1):
            T, C = TS[(k + 2 * mode + 1) % 5], CS[(k + mode) % 4]
            out.append(_random_case(i, N, (1, 3)[(k + mode) % 2], T, C, mode, ("scores", "weights")[(k // 2 + mode) % 2], (None, 0.5, 2.0)[(k + mode) % 3],
                                    poison=bool(k % 2)))
            i += 1
    out.append(_random_case(i, 3, 300, 5, 60, 1, "scores", 0.7)); i += 1                     # many clips: more than one workgroup per CU
    out.append(_random_case(i, 8, 4, 65, 60, 1, "scores", None, dead=0.4, poison=True)); i += 1   # dead slots between live ones
    out.append(_random_case(i, 33, 3, 64, 59, 0, "weights", None, dead=0.3)); i += 1
    out.append(_random_case(i, 64, 2, 64, 2, 1, "scores", 1.5)); i += 1                      # two classes: long runs of matches
    g = np.random.default_rng(77)
    full = [g.integers(0, 64, 64).tolist() for _ in range(3)]
    clips = [[list(full[n % 3]) if n % 5 else full[0][:63] for n in range(64)]]              # 64 hypotheses of 63 / 64 symbols
    out.append(build(f"{i}-N64-full-length", clips, 64, 64, 1, _scores(g, clips), None, 0.5)); i += 1
    same = [[[5, 9, 9, 2, 40]] * 5, [[]] * 5]
    out.append(build(f"{i}-identical", same, 7, 60, 1, [[-1, -2, -3, -4, -5]] * 2)); i += 1
    # hand-made: the top-1 stands alone, slots 1 and 2 agree: risk (2, 1, 1) under equal votes -> slot 1 (a tie between 1 and 2 as well)
    abc = [[[0, 1, 2], [0, 1, 3], [0, 1, 3]]]
    out.append(build(f"{i}-handmade-weights", abc, 5, 60, 0, None, [[1, 1, 1]])); i += 1
    out.append(build(f"{i}-handmade-scores", abc, 5, 60, 1, [[-1.0, -1.25, -1.25]], None, 1.0)); i += 1
    out.append(build(f"{i}-tie-of-two", [[[0, 1], [0, 2]]], 5, 60, 0, None, [[1, 1]])); i += 1
    out.append(build(f"{i}-all-votes-zero", [[[0, 1], [3], [0, 2, 2]]], 5, 60, 1, None, [[0, 0, 0]])); i += 1
    inf, nan = np.inf, np.nan
    four = [[[0, 1, 2, 3], [0, 1, 2], [0, 9, 2, 3], [4, 1, 2, 3]]] * 2
    out.append(build(f"{i}-scores-inf-nan", four, 6, 60, 1, [[-inf, -3, nan, -4], [nan, -inf, -inf, nan]], None, 2.0)); i += 1
    out.append(build(f"{i}-weights-neg-inf-nan", four, 6, 60, 0, None, [[-1, 2, inf, 0.5], [nan, 1, 1, -0.0]])); i += 1
    bad = [[[0, 1, 60], [0, 1]], [[0, 1, 2], [0, 1]], [[0, -7, 2], [3]], [[4, 4], [4, 59]]]
    out.append(build(f"{i}-symbol-outside", bad, 5, 60, 0, [[-1, -2]] * 4)); i += 1
    long_ = [[list(range(60)) + [1, 2, 3, 4, 5], [0, 1]], [[0, 1, 2], None], [None, list(range(50)) * 2], [None, None]]
    out.append(build(f"{i}-long-and-empty", long_, 100, 60, 1, [[-1, -2]] * 4)); i += 1
    out.append(build(f"{i}-long-and-symbol", [[[61] * 65, [0]]], 65, 60, 1, [[-1, -2]])); i += 1
    out.append(build(f"{i}-no-live-slot", [[None, None, None]], 5, 60, 0, [[0, 0, 0]])); i += 1
    g = np.random.default_rng(5)
    over = [[g.integers(0, 60, 5).tolist() for _ in range(4)]]
    out.append(build(f"{i}-length-clamped-to-T", over, 5, 60, 1, [[-1, -2, -2.5, -3]], raw_len=[[9, 5, 4096, 6]])); i += 1
    assert {c["N"] for c in out} >= set(NS) and {c["T"] for c in out} >= set(TS) and {c["C"] for c in out} >= set(CS)
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def case_lists(case):
    return mbr.nbest_to_lists(case["hyp_idx"], case["hyp_len"])


def _live_len(case):
    ln = np.minimum(case["hyp_len"].astype(np.int64), case["T"])
    return ln >= 0, np.where(ln >= 0, ln, -1)


def adhoc_case(name, hyp_idx, hyp_len, hyp_score, C, mode, inv_temp=None, weights=None):
    """a case from arrays that did not come from the table (the device's own n-best): `check` takes it as any other"""
    ix = np.ascontiguousarray(hyp_idx, np.int32)
    return dict(name=name, B=ix.shape[0], N=ix.shape[1], T=ix.shape[2], C=C, mode=mode, hyp_idx=ix, hyp_len=np.asarray(hyp_len, np.int32),
                hyp_score=None if hyp_score is None else np.asarray(hyp_score, np.float32), weights=None if weights is None else np.asarray(weights, np.float32),
                inv_temp=None if inv_temp is None else np.float32(inv_temp), adhoc=True)


@functools.lru_cache(maxsize=None)
def votes64(name):
    """(fp64 votes [B, N], x [B, N]: (s - s_max) * inv_temp where a score votes, 0 elsewhere) of a case of the table, computed once and read-only"""
    return votes64_of(next(c for c in cases() if c["name"] == name))


def votes64_of(c):
    name = c["name"]
    live, _ = _live_len(c)
    it = 1.0 if c["inv_temp"] is None else float(c["inv_temp"])
    w, x = np.zeros((c["B"], c["N"])), np.zeros((c["B"], c["N"]))
    for b in range(c["B"]):
        w[b] = mbr.votes_reference(live[b], None if c["hyp_score"] is None else c["hyp_score"][b], None if c["weights"] is None else c["weights"][b], it)
        if c["weights"] is None:
            s = c["hyp_score"][b].astype(np.float64)
            ok = live[b] & np.isfinite(s)
            if ok.any():
                x[b, ok] = (s[ok] - s[ok].max()) * it
    assert x.min() >= X_MIN, (name, x.min())
    w.setflags(write=False)
    x.setflags(write=False)
    return w, x


def check(case, got, k=K):
    """(failures, ratio) of a result against the three items of the module text"""
    B, N, T = case["B"], case["N"], case["T"]
    fails = []
    lists = case_lists(case)
    g = {key: np.asarray(got[key]) for key in ("out_idx", "out_len", "best", "risk", "w_out", "dist", "status")}
    assert g["risk"].dtype == np.float32 and g["w_out"].dtype == np.float32
    for b in range(B):
        best, risk, dist, status = mbr.mbr_reference(lists[b], mode=case["mode"], C=case["C"], votes=g["w_out"][b])
        if int(g["status"][b]) != status:
            fails.append(f"clip {b}: status {int(g['status'][b])}, reference {status}")
        if not np.array_equal(g["dist"][b], dist):
            fails.append(f"clip {b}: dist differs from the reference in {int((g['dist'][b] != dist).sum())} entries")
        if not np.array_equal(g["risk"][b].view(np.uint32), risk.view(np.uint32)):
            fails.append(f"clip {b}: risk is not the float32 recomputation from w_out: {g['risk'][b].tolist()} vs {risk.tolist()}")
        if int(g["best"][b]) != best:
            fails.append(f"clip {b}: best {int(g['best'][b])}, reference {best}")
        want = np.full(T, -1, np.int64)
        if best >= 0:
            want[:len(lists[b][best])] = lists[b][best]
        want_len = len(lists[b][best]) if best >= 0 else 0
        if int(g["out_len"][b]) != want_len or not np.array_equal(g["out_idx"][b], want):
            fails.append(f"clip {b}: out_idx / out_len are not slot {best} of the n-best")
    ref, x = votes64_of(case) if case.get("adhoc") else votes64(case["name"])
    w = g["w_out"].astype(np.float64)
    if case["weights"] is not None:
        ratio = 0.0
        if not np.array_equal(g["w_out"].view(np.uint32), ref.astype(np.float32).view(np.uint32)):
            fails.append("w_out is not the usable explicit weights (+0 elsewhere)")
            ratio = float("inf")
    else:
        zero = ref == 0
        if (w[zero] != 0).any() or np.signbit(g["w_out"][zero]).any():
            fails.append("a slot that must vote +0 votes")
        bound = ref * (2.0 * np.abs(x) + k) * EPS
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(zero, 0.0, np.abs(w - ref) / np.where(zero, 1.0, bound))
        ratio = float("inf") if not np.isfinite(w).all() else float(r.max()) if r.size else 0.0
        if ratio > 1.0:
            fails.append(f"w_out: err / bound {ratio:.3g}")
    return fails, ratio


# ---------------------------------------------------------------------------------------------------- the twin
_U = np.uint64
_ONE, _ALL = _U(1), _U(0xFFFFFFFFFFFFFFFF)


def _myers_pairs(peq, text, m, n, mutant):
    """Hyyro's bit-vector distance for P pairs at once: peq uint64 [P, 64] (the pattern's match masks), text uint8 [P, 64], m, n int [P]"""
    P = m.shape[0]
    pv, mv = np.full(P, _ALL), np.zeros(P, _U)
    mm = np.maximum(m, 1)
    top = _ONE << (mm - 1).astype(_U)
    if mutant == "top_bit_63":
        top = np.full(P, _ONE << _U(63))
    if mutant == "shift_by_64":                              # (1 << len) - 1 with a shifter that takes the amount modulo 64: no bits at len 64
        top = np.where(mm == 64, _U(0), top)
    score = m.astype(np.int64).copy()
    rows = np.arange(P)
    for kk in range(int(n.max()) if P else 0):
        on = kk < n
        eq = peq[rows, text[:, kk]]
        xv = eq | mv
        if mutant == "carry_dropped":                        # the 64-bit sum as two 32-bit sums without the carry between them
            lo = ((eq & pv) & _U(0xFFFFFFFF)) + (pv & _U(0xFFFFFFFF))
            hi = ((eq & pv) >> _U(32)) + (pv >> _U(32))
            s = (lo & _U(0xFFFFFFFF)) | (hi << _U(32))
        else:
            s = (eq & pv) + pv
        xh = (s ^ pv) | eq
        ph = mv | ~(xh | pv)
        mh = pv & xh
        score = score + np.where(on & ((ph & top) != 0), 1, 0) - np.where(on & ((mh & top) != 0), 1, 0)
        ph = (ph << _ONE) | (_U(0) if mutant == "first_row_zero" else _ONE)
        mh = mh << _ONE
        pv = np.where(on, mh | ~(xv | ph), pv)
        mv = np.where(on, ph & xv, mv)
    return np.where(m == 0, n, score)


def twin(case, mutant=None):
    """ishara_mbr_select in numpy with the kernel's arithmetic: match masks and Hyyro's recurrence in uint64, votes and risk in float32 with
    one rounding per operation.  `mutant`: one of MUTANTS, a mistake the checks must reject."""
    assert mutant is None or mutant in MUTANTS, mutant
    f32 = np.float32
    B, N, T, C, mode = case["B"], case["N"], case["T"], case["C"], case["mode"]
    out = dict(out_idx=np.full((B, T), -1, np.int32), out_len=np.zeros(B, np.int32), best=np.full(B, -1, np.int32), risk=np.full((B, N), np.nan, f32),
               w_out=np.zeros((B, N), f32), dist=np.full((B, N, N), -1, np.int32), status=np.zeros(B, np.int32))
    live_all, len_all = _live_len(case)
    it = f32(1.0) if case["inv_temp"] is None else f32(case["inv_temp"])
    with np.errstate(all="ignore"):
        for b in range(B):
            live, ln = live_all[b].copy(), len_all[b].copy()
            take = np.clip(ln, 0, 64)
            sym = np.zeros((N, 64), np.int64)
            ok = np.zeros((N, 64), bool)
            for n in range(N):
                sym[n, :take[n]] = case["hyp_idx"][b, n, :take[n]]
                ok[n, :take[n]] = (sym[n, :take[n]] >= 0) & (sym[n, :take[n]] < C)
            have = np.arange(64)[None, :] < take[:, None]
            status = (1 if (ln > 64).any() and mutant != "no_status_long" else 0) | (2 if (have & ~ok).any() else 0) | (0 if live.any() else 4)
            # votes
            voters = np.ones(N, bool) if mutant == "dead_slot_votes" else live
            w = np.zeros(N, f32)
            if case["weights"] is not None:
                v = case["weights"][b]
                use = voters & (v > 0) & (v < np.inf)
                w[use] = v[use]
            else:
                s = case["hyp_score"][b]
                fin = voters & (np.abs(s) < np.inf)
                if fin.any():
                    smax = f32(0.0) if mutant == "unshifted_scores" else s[fin].max()
                    w[fin] = np.exp(((s[fin] - smax).astype(f32) * it).astype(f32)).astype(f32)
            out["w_out"][b] = w
            out["status"][b] = status
            first = int(np.argmax(live)) if live.any() else -1
            best = first
            if not (status & 3) and first >= 0:
                lnv = np.where(voters, np.maximum(take, 0), -1)                      # a voting dead slot counts as an empty hypothesis
                text = np.where(ok, sym, 0).astype(np.uint8)
                peq = np.zeros((N, 64), _U)
                for n in range(N):
                    for kk in range(take[n]):
                        if ok[n, kk]:
                            peq[n, sym[n, kk]] |= _ONE << _U(kk)
                d = np.zeros((N, N), np.int64)
                if N > 1:
                    ii, jj = np.triu_indices(N, 1)
                    res = _myers_pairs(peq[ii], text[jj], np.maximum(lnv[ii], 0), np.maximum(lnv[jj], 0), mutant)
                    d[ii, jj] = res
                    d[jj, ii] = res
                pair = live[:, None] & live[None, :]
                out["dist"][b] = np.where(pair, d, -1)
                risk = np.full(N, np.nan, f32)
                order = range(N - 1, -1, -1) if mutant == "reverse_sum" else range(N)
                for i_ in range(N):
                    if not live[i_]:
                        continue
                    r = f32(0.0)
                    for j in order:
                        if not voters[j]:
                            continue
                        c = f32(d[i_, j])
                        if mode == 1:
                            c = f32(c / f32(max(int(take[i_] if mutant == "norm_by_candidate" else take[j]), 1)))
                        if mutant == "fma":
                            r = f32(np.float64(w[j]) * np.float64(c) + np.float64(r))
                        else:
                            r = f32(r + f32(w[j] * c))
                    risk[i_] = r
                out["risk"][b] = risk
                for i_ in range(first + 1, N):
                    if live[i_] and (risk[i_] <= risk[best] if mutant == "ties_to_higher" else risk[i_] < risk[best]):
                        best = i_
            out["best"][b] = best
            if best >= 0:
                bl = int(ln[best])
                out["out_len"][b] = bl
                out["out_idx"][b, :bl] = case["hyp_idx"][b, best, :bl]
    return out


def measure_k_host():
    """the worst (err / (ref * 2^-24) - 2 |x|) of the unmutated twin's votes over the table: K_HOST must not be below it"""
    worst = 0.0
    for c in cases():
        if c["weights"] is not None:
            continue
        ref, x = votes64(c["name"])
        w = twin(c)["w_out"].astype(np.float64)
        nz = ref > 0
        if nz.any():
            worst = max(worst, float((np.abs(w - ref)[nz] / (ref[nz] * EPS) - 2.0 * np.abs(x[nz])).max()))
    return worst
