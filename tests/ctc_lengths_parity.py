"""Helpers of tests/test_ctc_lengths_gpu.py and tests/test_ctc_lengths.py: the ragged cases of the four CTC kernels (per-sample frame
counts, the `*_ex` entry points), their references and the mistakes the cases are for.

A ragged case is a batch in a buffer of T frames in which sample b has its own count Tb = frame_len[b].  The labels and the logits come
from tests/ctc_parity.py (labels(), logits() of a Case with the same T: the whole buffer is N(0, 2^2), so the rows past a sample's end hold
ordinary finite values unless pad() overwrites them with NaN or +inf).

References
  primary   the existing fixed-T entry point launched on that sample alone at T = Tb (bit-equality; the GPU test does this);
  oracle()  oracle.ishara_oracle.ctc_nll in fp64 under autograd on x[b:b+1, :Tb] (samples of one Tb are run as one batch), the gradient
            past Tb exactly 0; a sample infeasible BY ITS OWN Tb by the kernel's contract (nll 1e30, gradient softmax on its Tb rows);
  restate() ctc_parity.restate per Tb on the slice, with the mistakes of MUTANTS applied by this wrapper (they concern which rows and
            which length a sample is given, not the recursions); with none it equals oracle() to 1e-9;
  the decoders and the aligner: O.decode_phrase / prefix_beam_search / viterbi_align of x[b, :Tb], or those with a mistake.
Bounds: ctc_parity's, unchanged (nll 1e-3 + 1e-5 |ref|, gradient grad_scale * 2e-5 + 1e-3 |ref|); compare() reports err / bound.
"""
import functools
from typing import NamedTuple

import numpy as np
import torch

import ctc_parity as P
from oracle import ishara_oracle as O

INT_FILL = 0x7F7F7F7F      # what an integer output holds before the launch (0xFF bytes would read as the -1 padding the kernels must write)


class Ragged(NamedTuple):
    name: str
    T: int
    C: int
    L: int
    blank: int
    samples: tuple          # of (Tb, len, repeats)
    seed: int = 0

    @property
    def B(self):
        return len(self.samples)

    @property
    def base(self):
        return P.Case(self.name, self.T, self.C, self.L, self.blank, tuple((n, rep) for _, n, rep in self.samples), seed=self.seed)


def labels(rc):
    return P.labels(rc.base)


def logits(rc):
    return P.logits(rc.base)


def frame_len(rc):
    return np.array([tb for tb, _, _ in rc.samples], np.int32)


def feasible(rc):
    n, rep = P.lengths(rc.base)
    return n + rep <= frame_len(rc)


def pad(x, fl, kind):
    """a copy of x [B, T, C] whose rows t >= fl[b] hold `kind`: "normal" (as drawn), "nan" or "inf" """
    x = np.array(x, np.float32)
    if kind != "normal":
        for b, tb in enumerate(fl):
            x[b, max(int(tb), 0):] = {"nan": np.nan, "inf": np.inf}[kind]
    return x


PADS = ("normal", "nan", "inf")


# ------------------------------------------------------------------ the loss cases
def tails():
    """group tails: one sample per Tb and label length; the alpha groups start at t = 1, the beta groups at Tb - 1, the gradient phase
    strides 16 frames per wave with four in flight"""
    L = 8
    s = tuple((tb, n, ()) for tb in P.B_TS for n in (0, min(1, tb), min(L, tb // 2), min(L, tb)))
    return Ragged("tails", 33, 60, L, 59, s, seed=2100)


def seams(L):
    """register seams in a buffer of 272 frames: every TIGHT sample that fits L with Tb = len + repeats (one alignment), one frame short
    (infeasible by its own length only: the buffer is long enough) and Tb = T; seam_samples(L) at Tb = 129, 130 and T"""
    T = 272
    s = []
    for n, rep in P.TIGHT:
        if n <= L:
            s += [(tb, n, rep) for tb in (n + len(rep), n + len(rep) - 1, T) if tb >= 1]
    for n, rep in P.seam_samples(L):
        s += [(tb, n, rep) for tb in (129, 130, T)]
    return Ragged(f"seams-L{L}", T, 60, L, 59, tuple(s), seed=2200 + L)


def tight_index(rc):
    """the samples with Tb = len + repeats: exactly one alignment"""
    return [b for b, (tb, n, rep) in enumerate(rc.samples) if tb == n + len(rep)]


def short_index(rc):
    """the samples one frame short of their label, in a buffer that would hold it"""
    return [b for b, (tb, n, rep) in enumerate(rc.samples) if tb == n + len(rep) - 1]


def contract():
    """feasible samples at the even positions; the odd ones get a frame_len outside [1, T] (BAD_LENGTHS)"""
    s = ((19, 9, (4,)), (19, 7, ()), (12, 12, ()), (19, 3, ()), (7, 0, ()), (19, 5, (2,)), (15, 7, ()), (19, 12, ()), (19, 2, ()))
    return Ragged("contract", 19, 60, 12, 59, s, seed=2300)


BAD_LENGTHS = (0, -3, 19 + 1, 2 ** 31 - 1)


def scaled():
    s = ((16, 5, ()), (9, 9, ()), (8, 8, ()), (16, 0, ()), (11, 4, (2,)), (5, 6, ()))        # the last: infeasible by its own length
    return Ragged("scaled", 16, 60, 12, 59, s, seed=2400)


SCALES_POW2 = np.array([0.25, 2.0, 1.0, 0.5, 8.0, 0.125], np.float32)
SCALES_ANY = np.array([0.3, 1.7, 37.5, 1 / 3, 0.01, 0.9], np.float32)


# ------------------------------------------------------------------ the loss references
def closed_form(rc, b):
    """(nll, gradient [Tb, C]) of a sample with exactly one alignment"""
    tb, n, rep = rc.samples[b]
    assert tb == n + len(rep)
    sm = P.softmax64(logits(rc)[b, :tb])
    p = P.path_of(labels(rc)[b], n, rc.blank, tb)
    g = sm.copy()
    g[np.arange(tb), p] -= 1.0
    return -np.log(sm[np.arange(tb), p]).sum(), g


def _by_length(fl):
    return {int(tb): np.nonzero(fl == tb)[0] for tb in np.unique(fl)}


@functools.lru_cache(maxsize=None)
def oracle(rc):
    """fp64 (nll [B], d nll / d logits [B, T, C]) of the oracle, sample by sample on its own rows; the contract for an infeasible sample"""
    x, y, fl, ok = logits(rc).astype(np.float64), labels(rc), frame_len(rc), feasible(rc)
    nll, grad = np.full(rc.B, 1e30), np.zeros_like(x)
    for tb, idx in _by_length(fl).items():
        xs = torch.from_numpy(x[idx, :tb]).requires_grad_(True)
        v = O.ctc_nll(torch.from_numpy(y[idx]), xs, rc.blank)
        v.sum().backward()
        nll[idx], grad[idx, :tb] = v.detach().numpy(), xs.grad.numpy()
    for b in np.nonzero(~ok)[0]:
        nll[b], grad[b, :fl[b]] = 1e30, P.softmax64(x[b, :fl[b]])
    return nll, grad


MUTANTS = {
    "beta_from_T": "the beta recursion started at T - 1: the gradient rows of a sample come from the recursions over all T rows of the buffer",
    "feasible_by_T": "feasibility judged by the buffer's T: a label that fits T but not Tb is run over T frames",
    "pad_rows_softmax": "gradient rows past Tb equal to grad_scale * softmax",
    "next_length": "frame_len[b + 1] used for sample b",
    "tail_group": "the last 8-group of a sample taken from the buffer's tail (rows T - 8 .. T - 1 in place of the group's own)",
    "scale_nll": "sample_scale applied to nll",
}
DECODE_MUTANTS = {
    "final_run_at_T": "greedy: the unemitted final run taken at T - 1, the frames up to T decoded",
    "frame_pos_unwritten": "align: frame_pos left as it was past Tb",
}


def restate(x, y, blank, fl, grad_scale=1.0, sample_scale=None, zero_inf=False, mut=()):
    """fp64 (nll [B], gradient [B, T, C]) of the ragged batch by ctc_parity.restate on each sample's own rows, by the *_ex contract, with
    the mistakes in `mut` (MUTANTS) applied.  x may hold NaN past a sample's end unless a mistake reads those rows."""
    assert set(mut) <= set(MUTANTS), mut
    x, y, fl = np.asarray(x, np.float64), np.asarray(y), np.asarray(fl).astype(np.int64)
    B, T, C = x.shape
    if "next_length" in mut:
        fl = np.concatenate([fl[1:], fl[-1:]])
    ss = np.ones(B) if sample_scale is None else np.asarray(sample_scale, np.float64)
    nll, grad = np.full(B, 1e30), np.zeros_like(x)
    n = (y != blank).sum(1)
    rep = np.array([int((y[b, 1:n[b]] == y[b, :max(n[b] - 1, 0)]).sum()) for b in range(B)])
    for tb, idx in _by_length(fl).items():
        if tb < 1 or tb > T:
            continue                                             # no frames: the sentinel, a zero gradient
        xs = x[idx, :tb].copy()
        if "tail_group" in mut and 1 < tb < T:
            g0 = 1 + 8 * ((tb - 2) // 8)                         # the alpha groups start at t = 1
            xs[:, g0:tb] = x[idx, T - (tb - g0):T]
        v, g = P.restate(xs, y[idx], blank, 1.0)
        if "beta_from_T" in mut:
            g = P.restate(x[idx], y[idx], blank, 1.0)[1][:, :tb]
        if "feasible_by_T" in mut:
            for k, b in enumerate(idx):
                if tb < n[b] + rep[b] <= T:
                    vv, gg = P.restate(x[b:b + 1], y[b:b + 1], blank, 1.0)
                    v[k], g[k] = vv[0], gg[0, :tb]
        nll[idx], grad[idx, :tb] = v, g
        if "pad_rows_softmax" in mut:
            grad[idx, tb:] = P.softmax64(x[idx, tb:])
    bad = nll >= P.SENTINEL
    if zero_inf:
        grad[bad] = 0.0
    grad *= (grad_scale * ss)[:, None, None]
    if "scale_nll" in mut:
        nll = np.where(bad, nll, nll * ss)
    return nll, grad


def compare(rc, nll, grad, grad_scale=1.0, sample_scale=None, zero_inf=False, ref=None, only=None):
    """nll [B], grad [B, T, C] or None against ref = (nll, unscaled gradient), oracle(rc) by default -> ({quantity: worst err / bound},
    failures).  Every sample (or those in `only`) and every element of the whole buffer is compared; an infeasible sample is held to the
    contract through the reference (oracle() states it), its nll to the sentinel.  A value that is not finite counts as an infinite error."""
    rn, rg = ref if ref is not None else oracle(rc)
    sel = np.arange(rc.B) if only is None else np.asarray(only)
    ss = np.ones(rc.B) if sample_scale is None else np.asarray(sample_scale, np.float64)
    nll = np.asarray(nll, np.float64)
    assert nll.shape == (rc.B,)
    inf = rn >= P.SENTINEL
    r = np.abs(nll - rn) / (P.NLL_ATOL + P.NLL_RTOL * np.abs(rn))
    r = np.where(inf, np.where(nll >= P.SENTINEL, 0.0, np.inf), np.where(np.isfinite(nll), r, np.inf))
    obs = {"nll": float(r[sel].max())}
    if grad is not None:
        grad = np.asarray(grad, np.float64)
        assert grad.shape == rg.shape
        gs = grad_scale * ss[:, None, None]
        want = np.where((inf & zero_inf)[:, None, None], 0.0, rg) * gs
        r = np.abs(grad - want) / (P.GRAD_ATOL * np.abs(gs) + P.GRAD_RTOL * np.abs(want))
        r = np.where(np.isfinite(grad), r, np.inf)
        obs["grad"] = float(r[sel].max())
    return obs, [f"{rc.name}: {q} err / bound = {v:.3g}" for q, v in obs.items() if not v <= 1.0]


# ------------------------------------------------------------------ greedy
DECODE_T = 513
DECODE_TBS = (1, 2, 3, 255, 256, 257, 258, 511, 512, 513)
DECODE_CS = (2, 17, 60)


def _from_argmax(g, a, Cc):
    """logits [T, C] whose argmax sequence is `a`: a margin of 1 over N(0, 0.01^2) noise (as tests/test_ctc_gpu.py builds them)"""
    x = (0.01 * g.standard_normal((len(a), Cc))).astype(np.float32)
    x[np.arange(len(a)), a] = np.float32(1.0)
    return x


@functools.lru_cache(maxsize=None)
def decode_batch(Cc):
    """(x [B, 513, C], frame_len [B], blank): per Tb two rows of runs of 1..3 frames.  Row 0 ends blank | class at Tb-2 | Tb-1 with a blank
    right after Tb-1: the run ending at Tb-1 is the unemitted one, and a decoder that looks past the end emits it.  Row 1 ends class | blank
    at Tb-2 | Tb-1: frame Tb-2 is the last one kept."""
    g = np.random.default_rng([4, Cc])
    blank = Cc - 1
    nb = [c for c in range(Cc) if c != blank]
    rows, fl = [], []
    for tb in DECODE_TBS:
        for form in (0, 1):
            a = []
            while len(a) < DECODE_T:
                a += [int(g.choice([blank, nb[g.integers(len(nb))]]))] * int(g.integers(1, 4))
            a = np.array(a[:DECODE_T])
            if tb >= 2:
                a[tb - 2] = blank if form == 0 else nb[0]
            a[tb - 1] = nb[0] if form == 0 else blank
            if form == 0:
                a[tb:tb + 1] = blank
            else:
                a[tb:] = nb[0]
            rows.append(_from_argmax(g, a, Cc))
            fl.append(tb)
    x = np.stack(rows)
    x.setflags(write=False)
    return x, np.array(fl, np.int32), blank


def decode_rows(x, fl, blank, mut=()):
    """(out_idx [B, T] int64 padded with -1, out_len [B]) of decode_phrase on each sample's own frames"""
    B, T, _ = x.shape
    idx, ln = np.full((B, T), -1, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        tb = T if "final_run_at_T" in mut else int(fl[b])
        if 1 <= tb <= T:
            w = O.decode_phrase(np.nan_to_num(x[b, :tb]), blank)
            idx[b, :len(w)], ln[b] = w, len(w)
    return idx, ln


# ------------------------------------------------------------------ beam
BEAM_T, BEAM_C, BM_CHUNK = 40, 20, 16
BEAM_TBS = (1, 3, 4, 5, BM_CHUNK - 1, BM_CHUNK, BM_CHUNK + 1, 2 * BM_CHUNK, 40)      # 3, 4, 5: the chunk of a one-wave launch is 4 frames
BEAM_WS = (1, 4, 32)


@functools.lru_cache(maxsize=None)
def beam_batch():
    """(x [B, 40, C], frame_len [B], lm [C, C] natural-log rows)"""
    g = np.random.default_rng(2500)
    x = (2 * g.standard_normal((len(BEAM_TBS), BEAM_T, BEAM_C))).astype(np.float32)
    t = g.standard_normal((BEAM_C, BEAM_C))
    lm = (t - np.log(np.exp(t).sum(1, keepdims=True))).astype(np.float32)
    x.setflags(write=False)
    return x, np.array(BEAM_TBS, np.int32), lm


# ------------------------------------------------------------------ align
ALIGN_LABELS = ((1, ()), (31, ()), (33, (32,)), (64, ()))      # (33, (32,)): labels 31 and 32 equal, the path steps 63 -> 64 -> 65


def align_case(T):
    """T = 64: the back-pointers in LDS, every label at Tb = len + repeats, one short, 9, 17 and T.  T = 1300: in the workspace, B = 3."""
    if T == 64:
        s = []
        for n, rep in ALIGN_LABELS:
            for tb in sorted({n + len(rep), n + len(rep) - 1, 9, 17, T}):
                if 1 <= tb <= T:
                    s.append((tb, n, rep))
        return Ragged("align-T64", 64, 60, 64, 59, tuple(s), seed=2600)
    return (Ragged("align-T1300-a", T, 60, 64, 59, ((T, 33, (32,)), (64, 64, ()), (9, 1, ())), seed=2601),
            Ragged("align-T1300-b", T, 60, 64, 59, ((33, 33, (32,)), (17, 31, ()), (T - 1, 64, ())), seed=2602))


def align_rows(x, y, fl, blank, mut=()):
    """viterbi_align of each sample's own frames in the batched layout: frame_pos [B, T] (-1 past Tb), start, end [B, L], conf, score (fp64)"""
    from ishara_amd.ctc_align import viterbi_align
    B, T, _ = x.shape
    L = y.shape[1]
    fp = np.full((B, T), INT_FILL if "frame_pos_unwritten" in mut else -1, np.int32)
    st, en = np.full((B, L), -1, np.int32), np.full((B, L), -1, np.int32)
    cf, sc = np.zeros((B, L)), np.full(B, -1e30)
    for b in range(B):
        tb = int(fl[b])
        if 1 <= tb <= T:
            f, st[b], en[b], cf[b], sc[b] = viterbi_align(np.nan_to_num(x[b, :tb]), y[b], blank)
            fp[b, :tb] = f
        else:
            fp[b] = -1
    return fp, st, en, cf, sc
