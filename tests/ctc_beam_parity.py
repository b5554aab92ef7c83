"""Cases, inputs, tracer and comparison for the CTC prefix beam search at its wave, chunk and merge edges (shared by test_ctc_beam_cases.py,
test_ctc_beam_mutants.py and test_ctc_beam_edges_gpu.py).

`trace` restates ishara_amd.ctc_beam.prefix_beam_search in fp64 with the same total order (score descending, then kind, source beam,
class) and carries what the kernel (csrc/ctc_beam.hip) carries besides: a trie node per prefix (new on every creation by extension), the
parent node recorded at creation, the owning wave rank % NW with its top-32 list, and the chunk index of each frame.  With twin=True every
stored quantity (log-softmax, pb, pnb, bonus, every lse) is carried a second time rounded to float32, on the candidates the fp64 run
selects; E is the largest |fp32 - fp64| candidate score.  Per row tau = max(8 E_row, 2^-17), at most 1e-3: two candidates each wrong by
E can swap across 2E, and the factor 8 leaves 4x for the device's expf / logf / log1pf differing from numpy's float32.  A clip is kept
only if its margin (as return_margin defines it, with nbest = W) exceeds tau, so every kept clip is decidable and the GPU test skips none;
every returned device score must lie within tau / 2 of the fp64 score.

Tie rows (TIE_CASES) stand beside the table: a candidate order that depends on the tie rule has margin 0 by definition, so no kept clip of
the table can see the tie order.  Their classes come in twins with identical logits in every frame: the tied candidates are computed by
the same operations on the same values, so the ties are exact in any precision, and every other gap (the smallest nonzero one) exceeds tau.
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple
from typing import List, Optional

import numpy as np

from ishara_amd.ctc_beam import CharBigramLM, _lm_rows, check_device_args
from ishara_amd.ctc_lm import CharNGramLM

NEG = -math.inf
TAU_MIN, TAU_MAX, TAU_FACTOR = 2.0 ** -17, 1e-3, 8.0
TIE_EPS = 1e-9           # tie rows: fp64 scores closer than this are one tie class (they are equal up to libm's lane-dependent last bit)
POOL = 4                 # clips drawn per kept clip: the acceptance share of a row is at least 1 / POOL


def waves(W: int) -> int:
    nw = 1
    while nw < W and nw < 16:
        nw *= 2
    return nw


def chunk(W: int) -> int:
    return min(16, 4 * waves(W))


MUTANTS = ("stale_no_merge", "loose_merge", "merged_tot_for_pb", "tie_order", "wave_first_beam_only", "wave_top16", "chunk_first_skipped",
           "chunk_first_twice", "tail_dropped", "lane32_dropped", "blank_last", "last_frame_ignored", "eos_dropped", "rank_before_eos",
           "nbest_beam_order", "len_is_T")

Trace = namedtuple("Trace", "hyps margin margin_full E counters")


def _lse(a, b, dt):
    a = np.asarray(a, dtype=dt)
    b = np.asarray(b, dtype=dt)
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.abs(a - b)
        r = m + np.log1p(np.exp(-d))
    return np.where(m == NEG, NEG, r).astype(dt)


def _log_softmax(x, dt):
    x = np.asarray(x, dtype=dt)
    m = x.max(axis=-1, keepdims=True)
    return ((x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=dt))).astype(dt)


def _numeric(dt, lpt, pb, pnb, last, msrc, b, C, mut):
    """The acoustic part of one frame in precision dt: pb' / pnb' of the same-prefix candidates (merged extensions folded in, the beam's
    own term first) and pnb' of every extension."""
    tot = _lse(pb, pnb, dt)
    s_pb = (tot + lpt[b]).astype(dt)
    s_pnb = np.where(last >= 0, pnb + lpt[np.maximum(last, 0)], NEG).astype(dt)
    for j in np.nonzero(msrc >= 0)[0]:
        i, c = int(msrc[j]), int(last[j])
        base = pb[i] if (last[i] == c and mut != "merged_tot_for_pb") else tot[i]
        s_pnb[j] = _lse(s_pnb[j], dt(base + lpt[c]), dt)
    e_pnb = (np.where(np.arange(C)[None, :] == last[:, None], pb[:, None], tot[:, None]) + lpt[None, :]).astype(dt)
    return s_pb, s_pnb, e_pnb


def _order(score, kind, src, cc, mut, tie_eps):
    if tie_eps > 0.0 and score.size:
        o = np.argsort(-score, kind="stable")
        cls = np.zeros(score.size, np.int64)
        cls[o] = np.concatenate([[0], np.cumsum(-np.diff(score[o]) > tie_eps)])
        first = cls
    else:
        first = -score
    if mut == "tie_order":
        return np.lexsort((kind, src, cc, first))
    return np.lexsort((cc, src, kind, first))


def _gap(hi, lo):
    return float(hi) - float(lo) if hi > lo else 0.0


def trace(logits, W: int, nbest: int = 1, lm=None, alpha: float = 0.0, beta: float = 0.0, blank: Optional[int] = None,
          mut: Optional[str] = None, twin: bool = False, tie_eps: float = 0.0) -> Trace:
    """One clip.  hyps: the n-best list [(indices, score)]; margin at this nbest and margin_full at nbest = W (tie_eps > 0: gaps inside a
    tie class do not count); E (twin only); counters (module docstring, test_ctc_beam_cases.py)."""
    x = np.asarray(logits, dtype=np.float64)
    T, C = x.shape
    b = C - 1 if (blank is None or mut == "blank_last") else int(blank)
    NW, ch = waves(W), chunk(W)
    table, nxt, start = _lm_rows(lm, C, b)
    use_lm = table is not None and alpha != 0.0
    f32 = np.float32
    lp = _log_softmax(x, np.float64)
    lp32 = _log_softmax(x.astype(f32), f32) if twin else None
    table32 = table.astype(f32) if (twin and table is not None) else None
    a32, b32 = f32(alpha), f32(beta)

    frames = list(range(T))
    if mut == "last_frame_ignored":
        frames = frames[:-1]
    elif mut == "chunk_first_skipped":
        frames = [t for t in frames if not (t > 0 and t % ch == 0)]
    elif mut == "chunk_first_twice":
        frames = [u for t in frames for u in ([t, t] if (t > 0 and t % ch == 0) else [t])]
    elif mut == "tail_dropped":
        frames = frames[:(T // ch) * ch]

    cnt = dict(merges=0, stale=0, second_beam_kept=0, frames_nb_lt_W=0, frames_cand_eq_W=0, frames_cand_gt_W=0, frames_cand_lt_W=0,
               merged_same_kept=0, last_frame_changes_top=0, eos_reorders=0, chunks=sorted({t // ch for t in frames}),
               ends_on_chunk=int(T % ch == 0), ends_past_chunk=int(T % ch == 1 and T > 1))
    margin = math.inf
    E = 0.0

    prefixes = [()]
    pb, pnb = np.zeros(1), np.full(1, NEG)
    lmsum, ln, last = np.zeros(1), np.zeros(1, np.int64), np.full(1, -1, np.int64)
    state = np.full(1, start, np.int64)
    node, par, nodes = np.zeros(1, np.int64), np.zeros(1, np.int64), 1
    pb32, pnb32, bonus32 = np.zeros(1, f32), np.full(1, NEG, f32), np.zeros(1, f32)
    for fi, t in enumerate(frames):
        nb = len(prefixes)
        top_before = prefixes[0]
        cnt["frames_nb_lt_W"] += int(nb < W)
        # 1. merge detection: true prefix identity (what the kernel's hash + node / chain comparison decides); stale = the child's recorded
        #    parent node is not the parent's current node
        msrc = np.full(nb, -1, np.int64)
        merged = np.zeros((nb, C), dtype=bool)
        index = {p: r for r, p in enumerate(prefixes)}
        for j in range(nb):
            if ln[j] == 0:
                continue
            c = int(last[j])
            if mut == "loose_merge":
                want = prefixes[j][-2] if ln[j] >= 2 else -1
                hit = [i for i in range(nb) if ln[i] == ln[j] - 1 and last[i] == want]
                for i in hit:
                    merged[i, c] = True
                if hit:
                    msrc[j] = hit[-1]
                continue
            i = index.get(prefixes[j][:-1])
            if i is None:
                continue
            stale = par[j] != node[i]
            if stale and mut == "stale_no_merge":
                continue
            cnt["merges"] += 1
            cnt["stale"] += int(stale)
            msrc[j] = i
            merged[i, c] = True
        # 2. candidates
        s_pb, s_pnb, e_pnb = _numeric(np.float64, lp[t], pb, pnb, last, msrc, b, C, mut)
        bonus = (alpha * lmsum if use_lm else 0.0) + beta * ln
        s_score = _lse(s_pb, s_pnb, np.float64) + bonus
        e_lm = lmsum[:, None] + table[state] if use_lm else np.zeros((nb, C))
        e_score = e_pnb + ((alpha * e_lm) if use_lm else 0.0) + beta * (ln[:, None] + 1)
        ok = ~merged & (e_score > NEG)
        ok[:, b] = False
        if mut == "lane32_dropped":
            ok[:, 32:] = False
        ei, ec = np.nonzero(ok)
        si = np.nonzero(s_score > NEG)[0]
        if twin:
            s_pb32, s_pnb32, e_pnb32 = _numeric(f32, lp32[t], pb32, pnb32, last, msrc, b, C, mut)
            s_score32 = _lse(s_pb32, s_pnb32, f32) + bonus32
            eb32 = ((bonus32[:, None] + a32 * table32[state]) if use_lm else np.broadcast_to(bonus32[:, None], (nb, C))) + b32
            e_score32 = e_pnb32 + eb32
            assert s_score32.dtype == f32 and e_score32.dtype == f32
            d = np.concatenate([np.abs(s_score32[si] - s_score[si]), np.abs(e_score32[ei, ec] - e_score[ei, ec])])
            E = max(E, float(d.max()) if d.size else 0.0)
        score = np.concatenate([s_score[si], e_score[ei, ec]])
        kind = np.concatenate([np.zeros(si.size, np.int64), np.ones(ei.size, np.int64)])
        src = np.concatenate([si, ei])
        cc = np.concatenate([np.zeros(si.size, np.int64), ec])
        order = _order(score, kind, src, cc, mut, tie_eps)
        n_cand = order.size
        cnt["frames_cand_lt_W"] += int(n_cand < W)
        cnt["frames_cand_eq_W"] += int(n_cand == W)
        cnt["frames_cand_gt_W"] += int(n_cand > W)
        if n_cand > W:
            g = _gap(score[order[W - 1]], score[order[W]])
            if not (tie_eps > 0.0 and g <= tie_eps):
                margin = min(margin, g)
        # 3. every wave keeps the top 32 of the beams it owns (rank % NW); the lists merge into the global order
        cut = 16 if mut == "wave_top16" else 32
        seen = np.zeros(NW, np.int64)
        keep = []
        for k in order:
            w = int(src[k]) % NW
            if mut == "wave_first_beam_only" and src[k] >= NW:
                continue
            if seen[w] < cut:
                seen[w] += 1
                keep.append(int(k))
                if len(keep) == W:
                    break
        # 4. the new beams
        n_pref, n_pb, n_pnb, n_lm, n_ln, n_last, n_state, n_node, n_par = [], [], [], [], [], [], [], [], []
        n_pb32, n_pnb32, n_bonus32 = [], [], []
        n_ext = 0
        for k in keep:
            s = int(src[k])
            cnt["second_beam_kept"] += int(s >= NW)
            if kind[k] == 0:
                cnt["merged_same_kept"] += int(msrc[s] >= 0)
                n_pref.append(prefixes[s]); n_pb.append(s_pb[s]); n_pnb.append(s_pnb[s])
                n_lm.append(lmsum[s]); n_ln.append(ln[s]); n_last.append(last[s]); n_state.append(state[s])
                n_node.append(node[s]); n_par.append(par[s])
                if twin:
                    n_pb32.append(s_pb32[s]); n_pnb32.append(s_pnb32[s]); n_bonus32.append(bonus32[s])
            else:
                c = int(cc[k])
                n_pref.append(prefixes[s] + (c,)); n_pb.append(NEG); n_pnb.append(e_pnb[s, c])
                n_lm.append(e_lm[s, c] if use_lm else 0.0); n_ln.append(ln[s] + 1); n_last.append(c)
                n_state.append(c if nxt is None else nxt[state[s], c])
                n_node.append(nodes + n_ext); n_par.append(node[s])
                n_ext += 1
                if twin:
                    n_pb32.append(NEG); n_pnb32.append(e_pnb32[s, c]); n_bonus32.append(eb32[s, c])
        nodes += n_ext
        prefixes = n_pref
        pb, pnb = np.array(n_pb, np.float64), np.array(n_pnb, np.float64)
        lmsum, ln, last = np.array(n_lm, np.float64), np.array(n_ln, np.int64), np.array(n_last, np.int64)
        state = np.array(n_state, np.int64)
        node, par = np.array(n_node, np.int64), np.array(n_par, np.int64)
        if twin:
            pb32, pnb32, bonus32 = np.array(n_pb32, f32), np.array(n_pnb32, f32), np.array(n_bonus32, f32)
        if fi == len(frames) - 1 and fi > 0:
            cnt["last_frame_changes_top"] = int(prefixes[0] != top_before)

    pre = _lse(pb, pnb, np.float64) + ((alpha * lmsum if use_lm else 0.0) + beta * ln)
    final = pre + alpha * table[state, b] if (use_lm and mut != "eos_dropped") else pre
    if twin:
        fin32 = _lse(pb32, pnb32, f32) + bonus32
        if use_lm:
            fin32 = fin32 + a32 * table32[state, b]
        E = max(E, float(np.abs(fin32 - final).max()))
    rank = np.arange(final.size)
    key = pre if mut == "rank_before_eos" else final
    zero = np.zeros(final.size, np.int64)
    order = rank if mut == "nbest_beam_order" else _order(key, zero, rank, zero, None, tie_eps)
    gaps = [_gap(final[order[k]], final[order[k + 1]]) for k in range(order.size - 1)]
    if tie_eps > 0.0:
        gaps = [g if g > tie_eps else math.inf for g in gaps]
    m_nb = min([margin] + gaps[:nbest])
    m_full = min([margin] + gaps[:W])
    o_pre = _order(pre, zero, rank, zero, None, tie_eps)
    cnt["eos_reorders"] = int(use_lm and list(o_pre[:nbest]) != list(order[:nbest]))
    hyps = [(np.array(prefixes[k], dtype=np.int64), float(final[k])) for k in order[:nbest]]
    return Trace(hyps, m_nb, m_full, E, cnt)


# --------------------------------------------------------------------------------------------------------------------------- the case table
Case = namedtuple("Case", "W T C blank nbest lm ex kind scale alpha beta B seed")


def _row(W, edge, C, blank, nbest, lm="none", ex=False, kind="rand", scale=8.0, B=8):
    c = chunk(W)
    T = {"1": 1, "c-1": c - 1, "c": c, "c+1": c + 1, "2c+1": 2 * c + 1}[edge]
    bl = {"last": C - 1, "0": 0, "mid": C // 2}[blank]
    nb = {"1": 1, "W": W, "mid": (W + 1) // 2}[nbest]
    alpha, beta = {"none": (0.0, 0.0), "table": (0.4, 0.5), "aut3": (0.5, 0.3)}[lm]
    return Case(W, T, C, bl, nb, lm, ex, kind, scale, alpha, beta, B, 0)


_ROWS = [
    # W = 1: NW 1, chunk 4
    _row(1, "1", 60, "last", "1"), _row(1, "c-1", 3, "0", "1", "table", scale=3.0), _row(1, "c", 64, "mid", "1", "aut3"),
    _row(1, "c+1", 2, "last", "1", scale=3.0), _row(1, "2c+1", 33, "0", "1", "table", kind="conf"),
    # W = 2: NW 2, chunk 8
    _row(2, "1", 2, "0", "W", scale=3.0), _row(2, "c-1", 5, "mid", "1", "aut3", scale=3.0), _row(2, "c", 60, "last", "W", "table"),
    _row(2, "c+1", 64, "0", "W", kind="conf"), _row(2, "2c+1", 3, "last", "W", "aut3", ex=True, scale=3.0),
    # W = 3: NW 4, a wave without a beam
    _row(3, "1", 5, "mid", "W", "table"), _row(3, "c-1", 33, "last", "mid"), _row(3, "c", 3, "0", "W", "aut3", scale=3.0),
    _row(3, "c+1", 60, "mid", "1"), _row(3, "2c+1", 64, "last", "W", "table"),
    # W = 4
    _row(4, "1", 64, "last", "W", "aut3"), _row(4, "c-1", 2, "0", "mid", scale=3.0), _row(4, "c", 5, "last", "W", scale=3.0),
    _row(4, "c+1", 33, "mid", "W", "table", kind="conf"), _row(4, "2c+1", 60, "last", "W", ex=True),
    # W = 5: NW 8
    _row(5, "1", 3, "last", "W"), _row(5, "c-1", 60, "0", "W", "aut3"), _row(5, "c", 64, "mid", "mid", "table"),
    _row(5, "c+1", 5, "0", "W", scale=3.0), _row(5, "2c+1", 3, "mid", "W", scale=3.0),
    # W = 8
    _row(8, "1", 33, "0", "mid", "table"), _row(8, "c-1", 64, "last", "W"), _row(8, "c", 2, "last", "W", "aut3", scale=3.0),
    _row(8, "c+1", 60, "last", "W", ex=True), _row(8, "2c+1", 3, "0", "W", "table", scale=3.0),
    # W = 15: NW 16
    _row(15, "1", 60, "mid", "W"), _row(15, "c-1", 5, "last", "W", "table", scale=3.0), _row(15, "c", 33, "0", "1"),
    _row(15, "c+1", 64, "last", "mid", "aut3"), _row(15, "2c+1", 5, "0", "W", scale=3.0),
    # W = 16: one beam per wave
    _row(16, "1", 5, "0", "W", "aut3"), _row(16, "c-1", 60, "last", "W", kind="conf"), _row(16, "c", 64, "0", "mid"),
    _row(16, "c+1", 33, "last", "W", "table"), _row(16, "2c+1", 3, "last", "W", "aut3", scale=3.0),
    # W = 17: wave 0 owns two beams, the others one
    _row(17, "1", 64, "mid", "W", "table"), _row(17, "c-1", 33, "mid", "W"), _row(17, "c", 60, "last", "mid", "aut3"),
    _row(17, "c+1", 5, "last", "1", scale=3.0), _row(17, "2c+1", 3, "0", "W", "table", ex=True, scale=3.0),
    # W = 24
    _row(24, "1", 33, "last", "W"), _row(24, "c-1", 3, "last", "mid", "table", scale=3.0), _row(24, "c", 64, "last", "W"),
    _row(24, "c+1", 60, "0", "W", "aut3"), _row(24, "2c+1", 5, "mid", "W", scale=3.0),
    # W = 31
    _row(31, "1", 60, "0", "1", "aut3"), _row(31, "c-1", 64, "0", "W", "table"), _row(31, "c", 5, "mid", "W", scale=3.0),
    _row(31, "c+1", 33, "last", "mid", kind="conf"), _row(31, "2c+1", 60, "last", "W", "table"),
    # W = 32: two beams per wave
    _row(32, "1", 64, "0", "W"), _row(32, "c-1", 60, "mid", "W", "aut3"), _row(32, "c", 33, "last", "W", "table"),
    _row(32, "c+1", 64, "last", "mid", "aut3", ex=True), _row(32, "2c+1", 3, "last", "W", scale=3.0),
    _row(32, "2c+1", 60, "last", "W"), _row(32, "2c+1", 5, "0", "W", "aut3", scale=3.0),
]
CASES = [c._replace(seed=1000 + k) for k, c in enumerate(_ROWS)]
# tie rows: classes in twins with identical logits (module docstring); no LM, so that the twin symmetry holds
TIE_CASES = [Case(4, 2, 5, 4, 4, "none", False, "twin", 3.0, 0.0, 0.0, 8, 2000), Case(17, 3, 7, 0, 17, "none", False, "twin", 3.0, 0.0, 0.0, 8, 2001),
             Case(32, 2, 64, 63, 32, "none", False, "twin", 3.0, 0.0, 0.0, 8, 2002)]


def case_id(c: Case) -> str:
    lm = {"none": "nolm", "table": "tab", "aut3": "aut3"}[c.lm]
    kind = "" if c.kind == "rand" and c.scale == 8.0 else ("-s3" if c.kind == "rand" else "-" + c.kind)
    return f"W{c.W}-T{c.T}-C{c.C}-blank{c.blank}-nb{c.nbest}-{lm}{'-ex' if c.ex else ''}{kind}"


def case_lm(c: Case):
    """The row's LM: None, a CharBigramLM (the table kernel) or an order-3 CharNGramLM (the automaton entry point)."""
    if c.lm == "none":
        return None
    g = np.random.default_rng(c.seed + 7)
    sym = [k for k in range(c.C) if k != c.blank]
    phrases = [[sym[int(v)] for v in g.integers(0, len(sym), int(g.integers(2, 12)))] for _ in range(120)]
    if c.lm == "table":
        return CharBigramLM.fit(phrases, num_classes=c.C, smoothing=0.5, blank=c.blank)
    return CharNGramLM.fit(phrases, order=3, num_classes=c.C, blank=c.blank)


def case_lengths(c: Case) -> np.ndarray:
    """Per-clip frame counts: T for a fixed-length row; an _ex row's batch hits 1, c, c + 1 and T (and c - 1, 2)."""
    if not c.ex:
        return np.full(c.B, c.T, np.int64)
    ch = chunk(c.W)
    cyc = [1, ch, ch + 1, c.T, ch - 1, 2]
    return np.array([min(cyc[k % len(cyc)], c.T) for k in range(c.B)], np.int64)


def confident(g, T, C, blank, sharp=8.0, noise=1.5):
    """As test_ctc_beam_gpu._confident: logits of a random alignment (runs of characters and blanks), ending in blank frames."""
    x = noise * g.standard_normal((T, C))
    end_blank = min(2, T - 1)
    sym = [k for k in range(C) if k != blank]
    t = 0
    while t < T - end_blank:
        n = int(g.integers(1, 5))
        c = blank if g.random() < 0.4 else sym[int(g.integers(0, len(sym)))]
        x[t:min(t + n, T - end_blank), c] += sharp
        t += n
    x[T - end_blank:, blank] += sharp
    return x


def _draw(g, c: Case):
    if c.kind == "conf":
        x = confident(g, c.T, c.C, c.blank)
    else:
        x = c.scale * g.standard_normal((c.T, c.C))
        if c.kind == "twin":                                # non-blank classes in pairs (k, k + h) with identical logits in every frame
            sym = [k for k in range(c.C) if k != c.blank]
            h = len(sym) // 2
            for k in range(h):
                x[:, sym[k + h]] = x[:, sym[k]]
    return x.astype(np.float32)


Built = namedtuple("Built", "case x lens lm expected margins E tau share counters E_clip")


@functools.lru_cache(maxsize=None)
def build(c: Case) -> Built:
    """Draws POOL * B clips from the row's seeded generator, E_row over all of them, tau_row from E_row; keeps the first B whose margin
    (nbest = W) exceeds tau_row.  x [B, T, C] float32 (frames past a clip's length are drawn too and must not matter)."""
    check_device_args(c.C, c.T, c.W, c.nbest)
    g = np.random.default_rng(c.seed)
    lm = case_lm(c)
    lens = case_lengths(c)
    tie_eps = TIE_EPS if c.kind == "twin" else 0.0
    pool = []
    for k in range(POOL * c.B):
        x = _draw(g, c)
        n = int(lens[k % c.B])
        pool.append((x, n, trace(x[:n], c.W, c.nbest, lm, c.alpha, c.beta, c.blank, twin=True, tie_eps=tie_eps)))
    E = max(p[2].E for p in pool)
    tau = min(max(TAU_FACTOR * E, TAU_MIN), TAU_MAX)
    share = sum(p[2].margin_full > tau for p in pool) / len(pool)
    # slot b of the batch takes the first clip of length lens[b] that is decidable
    xs, tr = [], []
    used = set()
    for b in range(c.B):
        for k, (x, n, r) in enumerate(pool):
            if k not in used and n == lens[b] and r.margin_full > tau:
                used.add(k)
                xs.append(x)
                tr.append(r)
                break
        else:
            raise AssertionError(f"{case_id(c)}: no decidable clip of length {lens[b]} among {len(pool)} draws (tau {tau:.3g})")
    return Built(c, np.stack(xs), lens, lm, [r.hyps for r in tr], [r.margin_full for r in tr], E, tau, share, [r.counters for r in tr],
                 [r.E for r in tr])


def expected(bt: Built, mut: Optional[str] = None) -> List[list]:
    """The n-best lists of the row's clips under a mistake of MUTANTS (None: the tracer as it is)."""
    c = bt.case
    tie_eps = TIE_EPS if c.kind == "twin" else 0.0
    out = []
    for b in range(c.B):
        n = c.T if mut == "len_is_T" else int(bt.lens[b])
        out.append(trace(bt.x[b, :n], c.W, c.nbest, bt.lm, c.alpha, c.beta, c.blank, mut=None if mut == "len_is_T" else mut, tie_eps=tie_eps).hyps)
    return out


def first_difference(ref, got, tol):
    """(slot, why) of the first slot where two n-best lists differ (symbols, or scores further apart than tol); None if none does."""
    for k in range(max(len(ref), len(got))):
        if k >= len(ref) or k >= len(got):
            return k, "list length"
        if list(ref[k][0]) != list(got[k][0]):
            return k, "symbols"
        if not abs(ref[k][1] - got[k][1]) <= tol:
            return k, "score"
    return None


def compare(bt: Built, idx, ln, sc):
    """The device's output (idx [B, nbest, T] int32, ln [B, nbest], sc [B, nbest] float32) against the row's expected lists: equal
    symbols and lengths, scores within tau / 2, -1 padding inside live slots, and (len -1, score -inf, indices -1) in every slot past the
    list.  Returns (observed worst score error, failure messages)."""
    c = bt.case
    bad, worst = [], 0.0
    for b in range(c.B):
        ref = bt.expected[b]
        got = [(idx[b, n, :max(ln[b, n], 0)].tolist(), float(sc[b, n])) for n in range(min(len(ref), c.nbest))]
        worst = max([worst] + [abs(r[1] - h[1]) for r, h in zip(ref, got) if list(r[0]) == h[0]])
        d = first_difference(ref, got, bt.tau / 2)
        if d is None and any(ln[b, n] != len(ref[n][0]) for n in range(len(ref))):
            d = (0, "length")
        if d is not None:
            k = d[0]
            bad.append(f"{case_id(c)} clip {b} (len {int(bt.lens[b])}, margin {bt.margins[b]:.3g}, tau {bt.tau:.3g}): slot {k} differs in {d[1]}: "
                       f"expected {ref[k][0].tolist() if k < len(ref) else None} {ref[k][1] if k < len(ref) else None!r}, "
                       f"got {got[k] if k < len(got) else None}")
            continue
        for n in range(len(ref)):
            if not (idx[b, n, ln[b, n]:] == -1).all():
                bad.append(f"{case_id(c)} clip {b} slot {n}: padding is not -1")
        n = len(ref)
        if not ((ln[b, n:] == -1).all() and np.isneginf(sc[b, n:]).all() and (idx[b, n:] == -1).all()):
            bad.append(f"{case_id(c)} clip {b}: slots past {n} are not (len -1, score -inf, indices -1)")
    return worst, bad
