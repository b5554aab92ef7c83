"""Helpers of tests/test_ctc_gpu.py and tests/test_ctc_mutants.py: the cases, the inputs, the fp64 references of the CTC loss kernel
(csrc/ctc.hip) with switchable mistakes, and the bounds.

Cases are built deterministically (a default_rng seed per case) from a description of each sample of the batch: its label length and the
positions i at which label i repeats label i-1 (every other neighbouring pair differs, where the class count allows it).  Label i is lattice
state 2i+1 and the kernel keeps state s in lane s % 64 of register s / 64, so labels 32k-1 and 32k (states 64k-1, 64k+1) sit on either side of
a register seam, and a label of 32k-1 / 32k / 32k+1 symbols ends the lattice (S = 2 len + 1 states) at 64k-1 / 64k+1 / 64k+3.

References
  oracle.ishara_oracle.ctc_nll in fp64 under autograd (pinned to torch.nn.functional.ctc_loss by tests/test_oracle_pins.py);
  closed_form(): a sample with T = len + repeats has one alignment, so nll = -sum_t log_softmax(x)[t, path_t], grad = softmax - onehot(path);
  restate(): the alpha / beta recursions as the kernel arranges them (bsum_t[s] = log-sum of the successors' betas, posterior =
  exp(alpha + bsum - log p)), in fp64, with the mistakes of MUTANTS switched on by name; with none it equals the oracle to 1e-9.

A sample is infeasible when T < len + repeats or a label lies outside [0, C): the kernel's contract (csrc/ctc.hip, include/ishara_hip.h) is
nll >= 1e29 and dlogits = grad_scale * softmax, all finite.  compare() holds such a sample to that contract and not to the oracle, whose
gradient there is autograd through the -1e30 sentinel.  (The C = 2 cases have one label class, so every label repeats its neighbour and the
31-, 32- and 40-symbol samples at T = 57 are infeasible.)

Bounds: those of tests/test_ops_gpu.py::test_ctc_and_decode for every logit regime -- nll |err| <= 1e-3 + 1e-5 |ref|, gradient
|err| <= grad_scale * 2e-5 + 1e-3 |ref| -- DESIGN.md §2 tabulates the err / bound observed on the MI355X per case group and regime.  compare() reports err / bound per
quantity (<= 1 passes).
"""
import functools
from typing import NamedTuple

import numpy as np
import torch

from oracle import ishara_oracle as O

NLL_RTOL, NLL_ATOL = 1e-5, 1e-3
GRAD_RTOL, GRAD_ATOL = 1e-3, 2e-5
SENTINEL = 1e29
REGIMES = ("n2", "n12", "flat", "shift", "dead", "trained")


class Case(NamedTuple):
    name: str
    T: int
    C: int
    L: int
    blank: int
    samples: tuple          # of (len, repeats): repeats = the positions i with label[i] == label[i-1]
    regime: str = "n2"
    seed: int = 0
    bad: tuple = ()         # of (sample, position, value): out-of-range label values written over the drawn ones

    @property
    def B(self):
        return len(self.samples)


# ------------------------------------------------------------------ the cases
def seam_samples(L):
    """lengths 0, 1, L; every 32k-1, 32k, 32k+1 <= L twice -- labels equal across each register seam below the length (the last six seams: at
    most six repeats), and different; one full-length sample with repeats away from every seam"""
    out = [(0, ()), (1, ()), (L, ())]
    for n in sorted({n for k in range(1, 9) for n in (32 * k - 1, 32 * k, 32 * k + 1) if n <= L}):
        out.append((n, tuple([32 * j for j in range(1, 8) if 32 * j < n][-6:])))
        out.append((n, ()))
    out.append((L, tuple(p for p in (3, 11, 20, 45, 77, 110) if p < L)))
    return tuple(out)


A_LS = (31, 32, 63, 64, 96, 128, 160, 192, 224, 255)
A_NS = (1, 2, 2, 3, 4, 5, 6, 7, 8, 8)


def case_a(L):
    return Case(f"A-L{L}", L + 13, 60, L, 59, seam_samples(L), seed=100 + L)


B_TS = (1, 2, 7, 8, 9, 10, 15, 16, 17, 18, 33)


def case_b(L, T):
    return Case(f"B-L{L}-T{T}", T, 60, L, 59, tuple((n, ()) for n in (0, min(1, T), min(L, T // 2), min(L, T))), seed=200 + L + T)


# one alignment only: (len, repeats); T = len + repeats.  (33, (32,)) and (255, (32, .., 224)) repeat across a seam: the path has to step
# 63 -> 64 -> 65 (the s-1 carry into lane 0); without the repeat it steps 63 -> 65 (the s-2 carry into lane 1)
TIGHT = ((1, ()), (31, ()), (31, (7,)), (32, ()), (33, ()), (33, (32,)), (64, ()), (64, (32, 40)), (255, ()), (255, (32, 64, 96, 128, 160, 192, 224)), (255, (100,)))


def case_c(i):
    n, rep = TIGHT[i]
    return Case(f"C-len{n}-rep{len(rep)}", n + len(rep), 60, n, 59, ((n, rep),), seed=300 + i)


def case_d(i):
    """the tight sample of case_c(i) one frame short (sample 1), between feasible samples"""
    n, rep = TIGHT[i]
    T = n + len(rep) - 1
    return Case(f"D-len{n}-rep{len(rep)}", T, 60, n, 59, ((T // 2, ()), (n, rep), (min(n, max(T - 2, 0)), ()), (0, ())), seed=400 + i)


D_IS = tuple(i for i in range(len(TIGHT)) if TIGHT[i][0] + len(TIGHT[i][1]) > 1)      # T >= 1
E_CB = ((2, 1), (2, 0), (5, 0), (33, 32), (60, 0), (60, 30), (64, 63), (64, 0))


def case_e(C, blank):
    return Case(f"E-C{C}-blank{blank}", 57, C, 40, blank, ((0, ()), (1, ()), (31, ()), (32, ()), (40, ()), (33, (32,))), seed=500 + 64 * C + blank)


F_SHAPES = ((64, 96), (255, 272))


def case_f(L, T, regime):
    return Case(f"F-L{L}-{regime}", T, 60, L, 59, seam_samples(L), regime=regime, seed=600 + L)


def case_g():
    return Case("G", 33, 60, 40, 59, ((0, ()), (1, ()), (16, (5,)), (31, ()), (33, ())), seed=700)


def case_h(C, T, infeasible):
    s = [(0, ()), (1, ()), (min(12, T // 2), (2,) if T >= 9 else ()), (min(33, T - 1), ())]
    if infeasible:
        s[1] = (T + 1, ())
    return Case(f"H-C{C}-T{T}-{'inf' if infeasible else 'ok'}", T, C, max(40, T + 1), C - 1, tuple(s), seed=800 + C + T)


def case_j(B):
    g = np.random.default_rng(900 + B)
    return Case(f"J-B{B}", 16, 60, 8, 59, tuple((int(g.integers(0, 9)), ()) for _ in range(B)), seed=900 + B)


def case_k(C, value, pos):
    """sample 1 holds one label outside [0, C) before its padding"""
    return Case(f"K-C{C}-v{value}-at{pos}", 19, C, 12, C - 1, ((9, (4,)), (7, ()), (12, ()), (0, ())), seed=1000 + C, bad=((1, pos, value),))


# ------------------------------------------------------------------ the inputs
@functools.lru_cache(maxsize=None)
def labels(case):
    """[B, L] int64 padded with blank"""
    g = np.random.default_rng([1, case.seed])
    cls = np.array([c for c in range(case.C) if c != case.blank])
    y = np.full((case.B, case.L), case.blank, np.int64)
    for b, (n, rep) in enumerate(case.samples):
        assert n <= case.L and all(0 < p < n for p in rep), case
        for i in range(n):
            if i > 0 and (i in rep or len(cls) == 1):
                y[b, i] = y[b, i - 1]
            else:
                c = cls if i == 0 else cls[cls != y[b, i - 1]]
                y[b, i] = c[g.integers(len(c))]
    for b, i, v in case.bad:
        y[b, i] = v
    y.setflags(write=False)
    return y


def lengths(case):
    y = labels(case)
    n = (y != case.blank).sum(1)
    rep = np.array([int((y[b, 1:n[b]] == y[b, :max(n[b] - 1, 0)]).sum()) for b in range(case.B)])
    return n, rep


def feasible(case):
    n, rep = lengths(case)
    y = labels(case)
    return (n + rep <= case.T) & ~((y < 0) | (y >= case.C)).any(1)


def path_of(y, n, blank, T):
    """one valid alignment of y[:n] over T >= n + repeats frames: the shortest one, its entries stretched as evenly as T allows"""
    m = []
    for i in range(n):
        if i > 0 and y[i] == y[i - 1]:
            m.append(blank)
        m.append(int(y[i]))
    if not m:
        return np.full(T, blank, np.int64)
    assert len(m) <= T
    reps = np.full(len(m), T // len(m))
    reps[:T % len(m)] += 1
    return np.repeat(np.array(m, np.int64), reps)


@functools.lru_cache(maxsize=None)
def logits(case):
    """[B, T, C] float32"""
    g = np.random.default_rng([2, case.seed, REGIMES.index(case.regime)])
    x = g.standard_normal((case.B, case.T, case.C))
    if case.regime == "n2":
        x *= 2
    elif case.regime == "n12":          # peaked
        x *= 12
    elif case.regime == "flat":         # near-uniform
        x *= 1e-3
    elif case.regime == "shift":
        x = 2 * x + 1000
    elif case.regime == "dead":         # a third of the classes (label classes among them) 80 below the rest
        x *= 2
        x[:, :, ::3] -= 80
    elif case.regime == "trained":      # +15 on one valid alignment's path over N(0, 1)
        y = labels(case)
        n, _ = lengths(case)
        for b in range(case.B):
            x[b, np.arange(case.T), path_of(y[b], n[b], case.blank, case.T)] += 15
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


# ------------------------------------------------------------------ the references
def _clean_labels(case):
    """the labels with out-of-range values replaced by a valid class (the oracle indexes with them; such a sample is infeasible anyway)"""
    y = labels(case).copy()
    y[(y < 0) | (y >= case.C)] = 0 if case.blank != 0 else 1
    return y


@functools.lru_cache(maxsize=None)
def reference(case):
    """fp64 (nll [B], d nll / d logits [B, T, C]) of the oracle"""
    x = torch.from_numpy(logits(case).astype(np.float64)).requires_grad_(True)
    nll = O.ctc_nll(torch.from_numpy(_clean_labels(case)), x, case.blank)
    nll.sum().backward()
    out = nll.detach().numpy(), x.grad.numpy()
    for a in out:
        a.setflags(write=False)
    return out


def softmax64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def closed_form(case):
    """a batch of samples with exactly one alignment each (T = len + repeats)"""
    y, x = labels(case), logits(case).astype(np.float64)
    n, rep = lengths(case)
    assert ((n + rep) == case.T).all(), case
    sm = softmax64(x)
    nll, grad = np.zeros(case.B), sm.copy()
    for b in range(case.B):
        p = path_of(y[b], n[b], case.blank, case.T)
        nll[b] = -np.log(sm[b, np.arange(case.T), p]).sum()
        grad[b, np.arange(case.T), p] -= 1.0
    return nll, grad


MUTANTS = {
    "skip_equal": "the s-2 transition allowed between equal labels",
    "a2_carry": "alpha: the s-2 carry dropped for states s mod 64 in {0, 1}",
    "a1_carry": "alpha: the s-1 carry dropped at s mod 64 = 0",
    "b2_carry": "beta: the s+2 carry dropped for states s mod 64 in {62, 63}",
    "b1_carry": "beta: the s+1 carry dropped at s mod 64 = 63",
    "final_no_sm2": "the final sum without alpha[S-2]",
    "S_full": "S = 2L+1: padding counted as labels",
    "empty_init1": "an empty label initialising (and accepting) state 1",
    "em_prev": "the emission of frame t-1",
    "skip_group_last": "the last frame of an 8-group (t = 8, 16, ..) skipped",
    "blank_last": "the blank fixed at C-1",
    "no_div_p": "the posterior not divided by p(y|x)",
    "scale_post_only": "grad_scale applied to the posterior only",
}


def restate(x, y, blank, grad_scale=1.0, mut=()):
    """fp64 (nll [B], grad_scale * d nll / d logits [B, T, C]) by the kernel's arrangement of the recursions, the mistakes in `mut` switched on.
    An infeasible sample comes out by the kernel's contract: nll 1e30, gradient grad_scale * softmax."""
    assert set(mut) <= set(MUTANTS), mut
    x, y = np.asarray(x, np.float64), np.asarray(y)
    B, T, C = x.shape
    L = y.shape[1]
    if "blank_last" in mut:
        blank = C - 1
    NEG = -np.inf
    sm = softmax64(x)
    lp = x - (x.max(-1, keepdims=True) + np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)))
    n = (y != blank).sum(1)
    SP = 2 * L + 1
    S = np.full(B, SP) if "S_full" in mut else 2 * n + 1
    ext = np.full((B, SP), blank, np.int64)
    ext[:, 1::2] = y
    s = np.arange(SP)[None, :]
    valid = s < S[:, None]
    some = (n > 0)[:, None]
    if "empty_init1" in mut:
        valid = valid | (s < 2)
        some = np.ones_like(some)
    bw2 = np.zeros((B, SP), bool)                                   # s-2 -> s
    bw2[:, 2:] = (ext[:, 2:] != blank) & ((ext[:, 2:] != ext[:, :-2]) | ("skip_equal" in mut))
    fw2 = np.zeros((B, SP), bool)                                   # s -> s+2
    fw2[:, :-2] = bw2[:, 2:]
    seam = s >= 64
    a1ok = np.ones((1, SP), bool) & ~(("a1_carry" in mut) & seam & (s % 64 == 0))
    a2ok = bw2 & ~(("a2_carry" in mut) & seam & (s % 64 <= 1))
    b1ok = np.ones((1, SP), bool) & ~(("b1_carry" in mut) & (s % 64 == 63))
    b2ok = fw2 & ~(("b2_carry" in mut) & (s % 64 >= 62))
    E = np.take_along_axis(lp, np.broadcast_to(ext[:, None, :], (B, T, SP)), 2)      # emission log-probabilities [B, T, SP]
    dead1, dead2 = np.full((B, 1), NEG), np.full((B, 2), NEG)
    with np.errstate(invalid="ignore", over="ignore"):
        A = np.full((B, T, SP), NEG)
        A[:, 0] = np.where(valid & ((s == 0) | ((s == 1) & some)), E[:, 0], NEG)
        for t in range(1, T):
            p = A[:, t - 1]
            if "skip_group_last" in mut and t % 8 == 0:
                A[:, t] = p
                continue
            a1 = np.where(a1ok, np.concatenate([dead1, p[:, :-1]], 1), NEG)
            a2 = np.where(a2ok, np.concatenate([dead2, p[:, :-2]], 1), NEG)
            A[:, t] = np.where(valid, np.logaddexp(np.logaddexp(p, a1), a2) + E[:, t - 1 if "em_prev" in mut else t], NEG)
        fin = (s == (S - 1)[:, None]) | ((s == (S - 2)[:, None]) & some & ("final_no_sm2" not in mut))
        if "empty_init1" in mut:
            fin = fin | ((n == 0)[:, None] & (s == 1))
        logp = np.logaddexp.reduce(np.where(fin & valid, A[:, T - 1], NEG), axis=1)
        Bs = np.full((B, T, SP), NEG)
        Bs[:, T - 1] = np.where(fin & valid, 0.0, NEG)
        for t in range(T - 2, -1, -1):
            b = Bs[:, t + 1] + E[:, t + 1]
            b1 = np.where(b1ok, np.concatenate([b[:, 1:], dead1], 1), NEG)
            b2 = np.where(b2ok, np.concatenate([b[:, 2:], dead2], 1), NEG)
            Bs[:, t] = np.where(valid, np.logaddexp(np.logaddexp(b, b1), b2), NEG)
        ok = np.isfinite(logp)
        st = A + Bs - (0.0 if "no_div_p" in mut else np.where(ok, logp, 0.0)[:, None, None])
        st = np.where(ok[:, None, None] & np.isfinite(st), np.exp(np.where(np.isfinite(st), st, NEG)), 0.0)
    onehot = (ext[:, :, None] == np.arange(C)[None, None, :]).astype(np.float64)
    post = np.einsum("bts,bsc->btc", st, onehot)
    grad = sm - grad_scale * post if "scale_post_only" in mut else grad_scale * (sm - post)
    return np.where(ok, -logp, 1e30), grad


# ------------------------------------------------------------------ the comparison
def compare(case, nll, grad, grad_scale=1.0, ref=None):
    """nll [B], grad [B, T, C] (None: nll only) against `ref` = (nll, unscaled gradient), the oracle's by default -> (observed {quantity: worst
    err / bound}, failures [text]).  Every sample and every element is compared; an infeasible sample is held to the contract (module
    docstring).  A value that is not finite counts as an infinite error."""
    rn, rg = ref if ref is not None else reference(case)
    ok = feasible(case)
    nll = np.asarray(nll, np.float64)
    assert nll.shape == (case.B,)
    obs, bad = {"nll": 0.0}, []
    r = np.abs(nll - rn) / (NLL_ATOL + NLL_RTOL * np.abs(rn))
    r = np.where(np.isfinite(nll), r, np.inf)
    if ok.any():
        obs["nll"] = float(r[ok].max())
    for b in np.nonzero(~ok)[0]:
        if not nll[b] >= SENTINEL:
            bad.append(f"{case.name}: infeasible sample {b}: nll {nll[b]:.6g} < 1e29")
    if grad is not None:
        grad = np.asarray(grad, np.float64)
        assert grad.shape == rg.shape, (grad.shape, rg.shape)
        want = np.where(ok[:, None, None], rg, softmax64(logits(case))) * grad_scale
        r = np.abs(grad - want) / (GRAD_ATOL * abs(grad_scale) + GRAD_RTOL * np.abs(want))
        r = np.where(np.isfinite(grad), r, np.inf)
        obs["grad"] = float(r[ok].max()) if ok.any() else 0.0
        if (~ok).any():
            obs["grad_infeasible"] = float(r[~ok].max())
    for q, v in obs.items():
        if not v <= 1.0:
            bad.append(f"{case.name}: {q} err / bound = {v:.3g}")
    return obs, bad
