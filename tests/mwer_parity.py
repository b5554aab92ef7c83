"""Shared by tests/test_mwer.py, tests/test_mwer_mutants.py and tests/test_mwer_gpu.py: the cases, the references and the bounds of
ishara_ctc_nbest_grad (csrc/ctc_nbest_grad.hip) and ishara_mwer_weights (csrc/mwer_weights.hip), and numpy twins with switchable mistakes.

Gradient cases (dict: name, logits float32 [B, T, C], blank, hyp_idx int32 [B, N, Th], hyp_len int32 [B, N], frame_len int32 [B] or None,
coef float32 [B, N], grad_scale, max_len), built like rescore_parity.score_cases and from its helpers.  A hypothesis is described by (len,
repeats); symbol i is lattice state 2 i + 1 and the kernels keep state s in lane s % 64 of register s / 64, so the lengths of SEAM_LENS put
S = 2 len + 1 on either side of 64, 128 and 512.
  reference   ishara_amd.mwer.nbest_grad_reference per clip on logits[b, :frame_len[b]] (fp64 alpha / beta posteriors), +0 past the end
  bound       |G - G_ref| <= |grad_scale| * sum_n |coef_n| * (GRAD_ATOL + GRAD_RTOL * |softmax - post_n|_ref) per element, n over the
              participating slots: each term is held to the loss kernel's own bound (tests/ctc_parity.py) scaled by its coefficient, per
              term because the terms cancel in the sum; the fp32 summation adds at most N * 2^-24 of sum |terms|, below it
  status      rescore_parity.expected_status with bit 3 also for hyp_len > max_len
  twin_grad() the definition arranged as the kernel (ctc_parity.restate's lattice per slot, n ascending), with the mistakes of GRAD_MUTANTS

Weight cases (dict: name, hyp_idx, hyp_len, logp float32 [B, N], status int32 [B, N] or None, targets int32 [B, L], inv_temp, mode).
  dist, tlen  exact, against ishara_amd.evaluation.levenshtein
  post        within ref * ((2 |x| + K) + max_j (2 |x_j| + K) + n) * 2^-24 * 1.001 of the fp64 posterior (rescore_parity's derivation: the
              vote bound (2 |x| + 5) * 2^-24 of mbr_parity on every e, the ascending sum, the division)
  risk, coef  bit-equal to recompute(): float32 numpy from the result's own post, one rounding per operation in the contract's order
  twin_weights() the same arithmetic in float32 with the mistakes of WEIGHT_MUTANTS
"""
import functools

import numpy as np

import ctc_parity as CP
import mbr_parity as MP
import rescore_parity as RP
from ishara_amd import mwer, rescore
from ishara_amd.evaluation import levenshtein

GRAD_RTOL, GRAD_ATOL = CP.GRAD_RTOL, CP.GRAD_ATOL
NLL_RTOL, NLL_ATOL = CP.NLL_RTOL, CP.NLL_ATOL
EPS, K, X_MIN = MP.EPS, MP.K, MP.X_MIN
SEAM_LENS = RP.SEAM_LENS
GRAD_MUTANTS = ("softmax_dropped", "coef_sign", "last_slot_skipped", "skip_equal", "frame_len_ignored")
WEIGHT_MUTANTS = ("risk_plain_mean", "no_inv_temp", "norm_by_hyp_len")
PAD = 59


# ------------------------------------------------------------------------------------------------ gradient cases
def make_coef(g, B, N):
    """rows with zeros (+0 and -0) and mixed signs; even rows sum to (nearly) 0, odd rows do not: only those expose a dropped softmax term"""
    c = g.standard_normal((B, N))
    for b in range(B):
        if N >= 3:
            c[b, g.integers(N)] = 0.0
        if b % 2 == 0 and N >= 2:
            c[b] -= c[b].sum() / N
            if N >= 3:
                z = int(np.argmin(np.abs(c[b])))
                c[b, (z + 1) % N] += c[b, z]
                c[b, z] = -0.0
        else:
            c[b] = np.abs(c[b]) + (0.0 if N >= 3 else 0.5)
            if N >= 3:
                c[b, g.integers(N)] = 0.0
    return c.astype(np.float32)


def grad_case(name, clips, T, C, blank, Th, seed, max_len, regime="n2", frame_len=None, poison=True, nan_past_end=False, coef=None,
              grad_scale=1.0):
    c = dict(RP.score_case(name, clips, T, C, blank, Th, seed, regime=regime, frame_len=frame_len, poison=poison, nan_past_end=nan_past_end))
    g = np.random.default_rng([11, seed])
    c["coef"] = make_coef(g, c["B"], c["N"]) if coef is None else np.asarray(coef, np.float32)
    c["coef"].setflags(write=False)
    c["grad_scale"], c["max_len"] = float(grad_scale), int(max_len)
    return c


@functools.lru_cache(maxsize=None)
def grad_cases():
    out = []
    g = np.random.default_rng(5100)
    C, bl = 8, 7
    H = lambda n, rep=(): RP.make_hyp(g, n, rep, C, bl)     # noqa: E731
    # the register seams at T <= 64, repeats on either side of the first seam
    out.append(grad_case("seams-64", [[H(0), H(1), H(31), H(32), H(33), H(63), H(64), H(33, (32,))]], 64, C, bl, 64, 1, 64))
    # ... and the long ones: S crosses 128 and 512; Th differs from T
    out.append(grad_case("seams-272", [[H(127), H(128), H(255), H(64, (32, 40))],
                                       [H(255, (32, 64, 96, 128, 160, 192, 224)), H(129, (127, 128)), H(65, (64,)), None]], 272, C, bl, 256, 2, 255,
                         grad_scale=0.5))
    # exactly one alignment (T_b = len + repeats: the gradient is softmax - onehot), one that does not fit, per clip through frame_len
    out.append(grad_case("tight", [[H(32), H(31, (7,)), H(30, (3, 9)), H(33), H(0)], [H(1), H(2), H(1), H(1), H(2, (1,))]], 40, C, bl, 40, 3, 40,
                         frame_len=[32, 1], nan_past_end=True, coef=[[0.5, -1.25, 2.0, 1.0, 0.75], [1.0, 3.0, -0.5, 0.25, 1.0]]))
    # ragged frame counts 0, 1, 17, T with NaN in every row past a clip's end
    rag = [[H(0), H(1), H(3, (1,)), None, H(5)]] * 4
    out.append(grad_case("ragged", rag, 33, C, bl, 12, 4, 12, frame_len=[0, 1, 17, 33], nan_past_end=True))
    for T in (1, 7, 8, 9, 17, 33):                           # the gather-ahead edges
        hs = [[H(min(T, 3), ()), H(0), H(min(T - 1, 2) if T > 1 else 0)], [H(1), H(min(T // 2, 5)), H(min(T, 2))]]
        out.append(grad_case(f"T{T}", hs, T, C, bl, max(T, 2), 10 + T, 8, grad_scale=2.0))
    out.append(grad_case("N1", [[H(5, (2,))], [H(0)]], 16, C, bl, 16, 30, 16, coef=[[1.0], [-2.0]]))
    out.append(grad_case("N4", [[H(3), H(4), H(2), H(6)], [H(1), H(2), H(3), H(4)]], 16, C, bl, 16, 31, 16))
    out.append(grad_case("N5", [[H(3), H(4), None, H(6), H(9, (1,))], [H(1), H(2), H(3), H(4), H(0)]], 16, C, bl, 16, 32, 16))
    n64 = [[RP.make_hyp(g, int(g.integers(0, 9)), (), C, bl) for _ in range(64)] for _ in range(2)]
    out.append(grad_case("N64", n64, 16, C, bl, 16, 33, 16))
    for Cn, b in ((2, 1), (60, 59), (64, 0)):
        gc = np.random.default_rng(5200 + Cn)
        hs = [[RP.make_hyp(gc, n, rep, Cn, b) for n, rep in ((0, ()), (1, ()), (7, (3,)) if Cn > 2 else (7, (1, 2, 3, 4, 5, 6)), (12, ()) if Cn > 2 else (3, (1, 2)))]]
        out.append(grad_case(f"C{Cn}-blank{b}", hs, 24, Cn, b, 24, 40 + Cn, 16))
    for r, regime in enumerate(("n12", "trained")):
        hs = [[H(20, (5,)), H(0), H(33, (32,)), H(12)], [H(8), H(33), H(2, (1,)), H(17)]]
        out.append(grad_case(f"regime-{regime}", hs, 48, C, bl, 48, 50 + r, 33, regime=regime))
    out.append(bad_slot_case())
    assert len({c["name"] for c in out}) == len(out)
    assert set(SEAM_LENS) <= {int(v) for c in out[:2] for v in c["hyp_len"].ravel()}
    return tuple(out)


def bad_slot_case():
    """a dead slot, a bad symbol, a slot longer than max_len, one longer than Th and one without an alignment among good ones"""
    g = np.random.default_rng(5300)
    C, bl, Th = 8, 7, 14
    H = lambda n, rep=(): RP.make_hyp(g, n, rep, C, bl)     # noqa: E731
    good = [[H(3), H(0), H(7, (2,)), H(5), H(9), H(2), H(1), H(4)], [H(6), H(2), H(0), H(10), H(3, (1, 2)), H(8), H(1), H(5)]]
    a = grad_case("bad-slots", good, 14, C, bl, Th, 60, 10, coef=np.where(np.arange(16).reshape(2, 8) % 3 == 0, -0.75, 1.5))
    idx, ln = a["hyp_idx"].copy(), a["hyp_len"].copy()
    idx[0, 1], ln[0, 1] = RP.DEAD_SYMBOL, -2
    idx[0, 3, :5] = [1, 2, 8, 3, 4]                          # a symbol == C
    idx[1, 1, :2] = [100000000, 1]
    idx[0, 5, :12], ln[0, 5] = RP.make_hyp(g, 12, (), C, bl), 12      # fits the frames and Th, longer than max_len = 10
    ln[1, 5] = 4000                                          # longer than Th
    idx[1, 6, :10], ln[1, 6] = RP.make_hyp(g, 10, (1, 2, 3, 4, 5), C, bl), 10      # 10 + 5 > 14 frames: no alignment
    for k in (idx, ln):
        k.setflags(write=False)
    return dict(a, hyp_idx=idx, hyp_len=ln)


def expected_status(case):
    st = RP.expected_status(case)
    ln = case["hyp_len"]
    return np.where((ln >= 0) & (ln > case["max_len"]), rescore.STATUS_LONG, st).astype(np.int32)


def participating(case):
    return (expected_status(case) == 0) & (case["coef"] != 0)


def hyp_of(case, b, n):
    return case["hyp_idx"][b, n, :case["hyp_len"][b, n]].tolist()


@functools.lru_cache(maxsize=None)
def grad_reference(name):
    """(G fp64 [B, T, C] with 0 past a clip's end, bound [B, T, C], logp fp64 [B, N] with -inf where the status is not 0)"""
    case = next(c for c in grad_cases() if c["name"] == name)
    return grad_reference_of(case)


def grad_reference_of(case):
    B, N, T, C = case["B"], case["N"], case["T"], case["C"]
    st = expected_status(case)
    G, bound, logp = np.zeros((B, T, C)), np.zeros((B, T, C)), np.full((B, N), -np.inf)
    for b in range(B):
        tb = RP.clip_frames(case, b)
        if tb < 1:
            continue
        hyps = [hyp_of(case, b, n) if st[b, n] == 0 else None for n in range(N)]
        g, a, lp = mwer.nbest_grad_reference(case["logits"][b, :tb].astype(np.float64), hyps, case["coef"][b], case["blank"], case["grad_scale"])
        G[b, :tb], logp[b] = g, lp
        part = participating(case)[b]
        bound[b, :tb] = abs(case["grad_scale"]) * (GRAD_ATOL * np.abs(case["coef"][b][part]).sum() + GRAD_RTOL * a)
    for k in (G, bound, logp):
        k.setflags(write=False)
    return G, bound, logp


def check_grad(case, G, ref=None):
    """(failures, worst err / bound) of G [B, T, C] against the fp64 reference; rows past a clip's end must be +0; an element whose bound is
    0 (a clip without a participating slot) must be 0"""
    rg, bound, _ = grad_reference(case["name"]) if ref is None else ref
    G = np.asarray(G)
    fails = []
    ratio = 0.0
    for b in range(case["B"]):
        tb = RP.clip_frames(case, b)
        tail = np.asarray(G[b, tb:], np.float32)
        if tail.size and (tail.view(np.uint32) != 0).any():
            fails.append(f"{case['name']}: clip {b}: a row past the clip's end is not +0")
        got = np.asarray(G[b, :tb], np.float64)
        if not np.isfinite(got).all():
            fails.append(f"{case['name']}: clip {b}: a gradient is not finite")
            ratio = np.inf
            continue
        err = np.abs(got - rg[b, :tb])
        bd = bound[b, :tb]
        zero = bd == 0
        if (err[zero] != 0).any():
            fails.append(f"{case['name']}: clip {b}: a clip without a participating slot has a gradient")
        if (~zero).any():
            ratio = max(ratio, float((err[~zero] / bd[~zero]).max()))
    if ratio > 1.0:
        fails.append(f"{case['name']}: gradient err / bound {ratio:.3g}")
    return fails, ratio


def label_rows(case, n, L=None):
    """hypothesis n of every clip, padded with blank, as the loss kernel's label rows int64 [B, L]; an empty row where the slot takes no part"""
    ok = expected_status(case)[:, n] == 0
    L = L or max(int(np.where(ok, case["hyp_len"][:, n], 0).max()), 1)
    y = np.full((case["B"], L), case["blank"], np.int64)
    for b in range(case["B"]):
        if ok[b]:
            y[b, :case["hyp_len"][b, n]] = hyp_of(case, b, n)
    return y, ok


def twin_grad(case, mutant=None):
    """the contract in fp64 as the kernel arranges it: per slot the lattice of ctc_parity.restate (softmax - post), n ascending, the frames
    of the clip only; one of GRAD_MUTANTS switched on"""
    assert mutant is None or mutant in GRAD_MUTANTS, mutant
    B, N, T, C = case["B"], case["N"], case["T"], case["C"]
    st = expected_status(case)
    G = np.zeros((B, T, C))
    last = N - 1 if mutant == "last_slot_skipped" else N
    for b in range(B):
        tb = RP.clip_frames(case, b)
        if mutant == "frame_len_ignored" and tb >= 1:
            tb = T
        if tb < 1:
            continue
        x = np.nan_to_num(case["logits"][b:b + 1, :tb].astype(np.float64))
        sm = CP.softmax64(x)[0]
        for n in range(last):
            cf = float(case["coef"][b, n])
            if st[b, n] != 0 or cf == 0.0:
                continue
            h = hyp_of(case, b, n)
            if tb < len(h) + RP.repeats_of(h):
                continue
            y = np.array([h + [case["blank"]]], np.int64)
            _, term = CP.restate(x, y, case["blank"], 1.0, ("skip_equal",) if mutant == "skip_equal" else ())
            term = term[0]
            if mutant == "softmax_dropped":
                term = term - sm
            G[b, :tb] += (-cf if mutant == "coef_sign" else cf) * term
    return case["grad_scale"] * G


# ------------------------------------------------------------------------------------------------ weight cases
def weight_case(name, clips, targets, seed, inv_temp=None, mode=1, status=None, logp=None, Th=None, spread=4.0):
    g = np.random.default_rng([13, seed])
    B, N = len(clips), len(clips[0])
    Th = Th or max(max((len(h) for hs in clips for h in hs if h is not None), default=1), 1) + 2
    idx, ln = RP.pack(clips, Th, poison=True)
    L = max(max(len(t) for t in targets), 1)
    tg = np.full((B, L), PAD, np.int32)
    for b, t in enumerate(targets):
        tg[b, :len(t)] = t
    lp = (-np.abs(g.standard_normal((B, N))) * spread - 3.0).astype(np.float32) if logp is None else np.asarray(logp, np.float32)
    return dict(name=name, hyp_idx=idx, hyp_len=ln, logp=lp, status=None if status is None else np.asarray(status, np.int32), targets=tg,
                inv_temp=None if inv_temp is None else np.float32(inv_temp), mode=mode, B=B, N=N, Th=Th, L=L)


@functools.lru_cache(maxsize=None)
def weight_cases():
    out = []
    g = np.random.default_rng(5400)
    C, bl = 59, 58
    H = lambda n: RP.make_hyp(g, n, (), C, bl)              # noqa: E731

    def near(t, k):                                          # the target with k random edits
        h = list(t)
        for _ in range(k):
            op, pos = int(g.integers(3)), int(g.integers(len(h) + 1))
            if op == 0 and h:
                h.pop(min(pos, len(h) - 1))
            elif op == 1:
                h.insert(pos, int(g.integers(C)))
            elif h:
                h[min(pos, len(h) - 1)] = int(g.integers(C))
        return h

    t0, t1, t2 = H(12), H(30), H(64)
    out.append(weight_case("basic", [[near(t0, k) for k in (0, 1, 2, 5)], [near(t1, k) for k in (3, 0, 7, 1)]], [t0, t1], 1))
    out.append(weight_case("temperature-plain", [[near(t0, k) for k in (0, 1, 2, 5, 9)], [near(t1, k) for k in (3, 0, 7, 1, 2)]], [t0, t1], 2,
                           inv_temp=0.5, mode=0))
    out.append(weight_case("sharp", [[near(t1, k) for k in (4, 2, 0)], [near(t0, k) for k in (1, 6, 3)]], [t1, t0], 3, inv_temp=3.0, spread=2.0))
    # the target's 64 symbols fill the word; hypotheses longer than the target; the empty hypothesis; an empty target (tlen 0: divide by 1)
    out.append(weight_case("L64", [[near(t2, 0), near(t2, 9), H(90), []], [H(3), [], H(1), H(70)]], [t2, []], 4))
    dead = [[near(t0, 1), None, near(t0, 3), near(t0, 2), None, near(t0, 0)], [None] * 6, [near(t1, 2)] + [None] * 5]
    lp = (-np.abs(g.standard_normal((3, 6))) * 3 - 2).astype(np.float32)
    lp[0, 2], lp[0, 3] = -np.inf, np.nan                     # not finite: not live
    st = np.zeros((3, 6), np.int32)
    st[0, 5] = 2                                             # a status: not live
    out.append(weight_case("dead-slots-and-a-clip-without-a-live-slot", dead, [t0, t0, t1], 5, status=st, logp=lp))
    n64 = [[near(t0, int(g.integers(0, 8))) for _ in range(64)]]
    out.append(weight_case("N64", n64, [t0], 6, inv_temp=0.25))
    out.append(weight_case("N1", [[near(t0, 2)], [None]], [t0, t1], 7))
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def live_of(case):
    lp = case["logp"]
    st = np.zeros_like(case["hyp_len"]) if case["status"] is None else case["status"]
    return (case["hyp_len"] >= 0) & (st == 0) & np.isfinite(lp)


def weights_reference(case):
    """dist int64 [B, N], tlen [B], fp64 post [B, N] and x [B, N] (the exponent; 0 where not live)"""
    B, N = case["B"], case["N"]
    live = live_of(case)
    it = 1.0 if case["inv_temp"] is None else float(case["inv_temp"])
    dist, tlen = np.full((B, N), -1, np.int64), np.zeros(B, np.int64)
    post, xs = np.zeros((B, N)), np.zeros((B, N))
    for b in range(B):
        tgt = rescore.target_symbols(case["targets"][b])
        tlen[b] = len(tgt)
        for n in range(N):
            if live[b, n]:
                h = case["hyp_idx"][b, n, :min(case["hyp_len"][b, n], case["Th"])].tolist()
                dist[b, n] = levenshtein([int(v) for v in h], tgt)
        if live[b].any():
            s = case["logp"][b].astype(np.float64)
            x = (s[live[b]] - s[live[b]].max()) * it
            assert x.min() >= X_MIN, (case["name"], x.min())
            e = np.exp(x)
            post[b, live[b]], xs[b, live[b]] = e / e.sum(), x
    return dist, tlen, post, xs


def recompute(case, dist, tlen, post, mutant=None):
    """(risk float32 [B], coef float32 [B, N]) from post in float32, one rounding per operation, in the contract's order"""
    assert mutant is None or mutant in WEIGHT_MUTANTS, mutant
    f32 = np.float32
    B, N = case["B"], case["N"]
    live = live_of(case)
    it = f32(1.0) if case["inv_temp"] is None else f32(case["inv_temp"])
    risk, coef = np.zeros(B, f32), np.zeros((B, N), f32)
    post = np.asarray(post, f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            W = np.asarray(dist[b], np.int64).astype(f32)
            if case["mode"] == 1:
                if mutant == "norm_by_hyp_len":
                    W = (W / np.maximum(case["hyp_len"][b], 1).astype(f32)).astype(f32)
                else:
                    W = (W / f32(max(int(tlen[b]), 1))).astype(f32)
            if not live[b].any():
                risk[b] = np.nan
                continue
            r = f32(0.0)
            for n in range(N):
                if live[b, n]:
                    r = f32(r + f32(post[b, n] * W[n]))
            risk[b] = r
            base = f32(W[live[b]].astype(np.float64).mean()) if mutant == "risk_plain_mean" else r
            for n in range(N):
                if live[b, n]:
                    v = f32(post[b, n] * f32(W[n] - base))
                    coef[b, n] = -v if mutant == "no_inv_temp" else -f32(it * v)
    return risk, coef


def check_weights(case, got):
    """(failures, worst posterior err / bound) of a result dict(dist, post, risk, coef, tlen)"""
    dist, tlen, post, xs = weights_reference(case)
    live = live_of(case)
    fails, worst = [], 0.0
    if not np.array_equal(np.asarray(got["dist"], np.int64), dist):
        fails.append(f"dist {np.asarray(got['dist']).tolist()} != {dist.tolist()}")
    if not np.array_equal(np.asarray(got["tlen"], np.int64), tlen):
        fails.append(f"tlen {np.asarray(got['tlen']).tolist()} != {tlen.tolist()}")
    p = np.asarray(got["post"], np.float32)
    if (p[~live].view(np.uint32) != 0).any():
        fails.append("a slot that is not live has a posterior that is not +0")
    if (np.asarray(got["coef"], np.float32)[~live].view(np.uint32) != 0).any():
        fails.append("a slot that is not live has a coef that is not +0")
    for b in range(case["B"]):
        lv = live[b]
        if not lv.any():
            continue
        d = (2.0 * np.abs(xs[b, lv]) + K) * EPS
        bound = post[b, lv] * (d + d.max() + int(lv.sum()) * EPS) * 1.001
        r = np.abs(p[b, lv].astype(np.float64) - post[b, lv]) / bound
        worst = max(worst, float(np.where(np.isfinite(p[b, lv]), r, np.inf).max()))
    if worst > 1.0:
        fails.append(f"posterior err / bound {worst:.3g}")
    risk, coef = recompute(case, got["dist"], got["tlen"], p)
    if not np.array_equal(np.asarray(got["risk"], np.float32).view(np.uint32), risk.view(np.uint32)):
        fails.append(f"risk {np.asarray(got['risk']).tolist()} is not the float32 recomputation {risk.tolist()}")
    if not np.array_equal(np.asarray(got["coef"], np.float32).view(np.uint32), coef.view(np.uint32)):
        fails.append("coef is not the float32 recomputation from post")
    return fails, worst


def twin_weights(case, mutant=None):
    """ishara_mwer_weights in float32 numpy (exact distances, numpy's float32 exp), one of WEIGHT_MUTANTS switched on"""
    f32 = np.float32
    dist, tlen, _, _ = weights_reference(case)
    live = live_of(case)
    it = f32(1.0) if case["inv_temp"] is None else f32(case["inv_temp"])
    post = np.zeros((case["B"], case["N"]), f32)
    for b in range(case["B"]):
        if live[b].any():
            mx = case["logp"][b][live[b]].max()
            e = np.where(live[b], np.exp((np.where(live[b], case["logp"][b] - mx, 0).astype(f32) * it).astype(f32)).astype(f32), f32(0))
            tot = f32(0.0)
            for n in range(case["N"]):
                if live[b, n]:
                    tot = f32(tot + e[n])
            post[b] = np.where(live[b], (e / tot).astype(f32), f32(0))
    risk, coef = recompute(case, dist, tlen, post, mutant)
    return dict(dist=dist, tlen=tlen, post=post, risk=risk, coef=coef)
