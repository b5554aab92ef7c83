"""Shared by the edit-alignment tests (no tests here): the case table, its packing into the device layout, the host reference on that
layout (evaluation.edit_alignment behind the entry's clamp and fallback rules) and the exact comparator.

The cases are the smallest shapes at which csrc/score_align.hip can go wrong: both sides of the len < 3 fallback, the 64-row chunk edges
of its walk, a full row, empty / one-symbol / all-lanes targets, L < 64 (unused lanes), small alphabets (ties: the move order decides),
prefix and suffix relations (all insertions trailing / leading, all deletions trailing / leading), the rows pinned by hand, lengths
outside 0..T and prediction symbols outside 0..58."""
import functools
from typing import List, NamedTuple

import numpy as np

from ishara_amd.evaluation import edit_alignment
from ishara_amd.tflite_model import FALLBACK_PHRASE

PAD = 59
SHAPES = [(384, 64), (8, 64), (384, 40), (8, 40), (384, 1), (8, 1)]      # (T, L)

# (a, b, ops, aligned, inserted): worked out by hand from the move order diagonal, up, left
PINNED = [
    ([1, 1], [1], (1, 0, 0, 1), [1], [1, 0]),
    ([1], [1, 1], (1, 0, 1, 0), [-1, 1], [0, 0, 0]),
    ([1, 2, 3], [3, 1, 2], (2, 0, 1, 1), [-1, 1, 2], [0, 0, 0, 1]),
    ([5, 6], [6, 5], (0, 2, 0, 0), [5, 6], [0, 0, 0]),
]

# pairs whose walk reaches a cell where the diagonal does not apply and both up and left do (rare: found by search over three symbols)
UP_AND_LEFT = [
    ([0, 0, 2, 0, 2], [0, 2, 0, 2, 2]),
    ([0, 0, 1, 0, 2, 1], [0, 0, 0, 1, 1, 2]),
    ([1, 0, 2, 2, 1, 2], [2, 1, 1, 2, 2]),
    ([1, 1, 0, 0, 1, 0], [1, 1, 2, 1, 0, 1]),
]


class Case(NamedTuple):
    name: str
    pred: np.ndarray        # the symbols in the idx row (the rest of the row is -1)
    out_len: int            # as passed: may lie outside 0..T
    target: np.ndarray      # before padding


@functools.lru_cache(maxsize=None)
def cases(T: int, L: int) -> List[Case]:
    g = np.random.default_rng(1000 * T + L)
    out: List[Case] = []

    def add(name, pred, target, out_len=None):
        pred, target = np.asarray(pred, np.int64)[:T], np.asarray(target, np.int64)[:L]
        out.append(Case(name, pred, len(pred) if out_len is None else out_len, target))

    nbs = sorted({n for n in (0, 1, 2, 63, 64, L) if n <= L})
    small = [n for n in (0, 1, 2, 3, 5) if n <= T]
    large = sorted({n for n in (63, 64, 65, 128, 129, T - 1, T) if 5 < n <= T})
    for na in small:                                        # both sides of the fallback against every target length
        for nb in nbs:
            add(f"na{na}-nb{nb}", g.integers(0, 59, na), g.integers(0, 59, nb))
    for k, na in enumerate(large):                          # chunk edges and the full row: all lanes, and one of the short targets
        for nb, alpha in ((nbs[-1], 59 if k % 2 else 3), (nbs[k % len(nbs)], 3 if k % 2 else 59)):
            add(f"na{na}-nb{nb}-alpha{alpha}", g.integers(0, alpha, na), g.integers(0, alpha, nb))
    for nb in sorted({1, min(7, L), L}):                    # identical sequences
        if nb <= T:
            t = g.integers(0, 59, nb)
            add(f"identical{nb}", t, t)
    for alpha in (2, 3):                                    # ties dominate: the move order is what is tested
        for _ in range(6):
            add(f"alpha{alpha}", g.integers(0, alpha, g.integers(0, min(T, 12) + 1)), g.integers(0, alpha, g.integers(0, min(L, 9) + 1)))
    n = min(T, L)
    t = g.integers(0, 4, n)
    k = max(n // 2, 1) if n > 1 else 0
    add("target-is-prefix", t, t[:k])                       # insertions, all trailing
    add("target-is-suffix", t, t[n - k:])                   # insertions, all leading
    add("pred-is-prefix", t[:k], t)                         # deletions, all trailing
    add("pred-is-suffix", t[n - k:], t)                     # deletions, all leading: the walk reaches i == 0 with j left
    for a, b, *_ in PINNED:
        add("pinned", a, b)
    for a, b in UP_AND_LEFT:
        add("up-and-left", a, b)
    full = g.integers(0, 5, T)
    add("len-negative", full[:min(T, 6)], g.integers(0, 5, min(L, 4)), out_len=-3)
    add("len-past-T", full, g.integers(0, 5, min(L, 7)), out_len=T + 5)
    add("symbols-59-60", [3, 59, 60, 4, 3, 59][:T], [3, 4, 3, 7][:L])
    add("symbols-59-60-no-target", [60, 59, 2, 59][:T], [])
    return out


def pack(cs: List[Case], T: int, L: int):
    """(idx int32 [B, T] padded with -1, out_len int32 [B], targets int32 [B, L] padded with 59)"""
    B = len(cs)
    idx, ln, tg = np.full((B, T), -1, np.int32), np.zeros(B, np.int32), np.full((B, L), PAD, np.int32)
    for b, c in enumerate(cs):
        idx[b, :len(c.pred)] = c.pred
        ln[b] = c.out_len
        tg[b, :len(c.target)] = c.target
    return idx, ln, tg


def prediction(idx_row: np.ndarray, out_len: int, T: int, fallback: bool) -> List[int]:
    """What the entry aligns: out_len clamped to 0..T, then the len < 3 rule when fallback is set."""
    n = min(max(int(out_len), 0), T)
    return [int(x) for x in FALLBACK_PHRASE] if (fallback and n < 3) else [int(x) for x in idx_row[:n]]


def sym(x: int) -> int:
    return x if 0 <= x < PAD else PAD


def reference_of(idx, ln, tg, fallback: bool, align=edit_alignment):
    """(ops [B, 4], aligned [B, L], inserted [B, L + 1], confusion [60, 60]) int64 of the packed arrays, by the host reference"""
    B, T = idx.shape
    L = tg.shape[1]
    ops, aligned, inserted = np.zeros((B, 4), np.int64), np.full((B, L), -2, np.int64), np.zeros((B, L + 1), np.int64)
    conf = np.zeros((60, 60), np.int64)
    for b in range(B):
        al = align(prediction(idx[b], ln[b], T, fallback), tg[b])
        nb = al.aligned.shape[0]
        ops[b] = al.ops
        aligned[b, :nb] = al.aligned
        inserted[b, :nb + 1] = al.inserted
        for t, p in al.pairs:
            conf[sym(t), sym(p)] += 1
    return ops, aligned, inserted, conf


@functools.lru_cache(maxsize=None)
def reference(T: int, L: int, fallback: bool):
    """The reference outputs of the whole table at (T, L): computed once, shared, never modified (the arrays are read-only)."""
    out = reference_of(*pack(cases(T, L), T, L), fallback)
    for a in out:
        a.setflags(write=False)
    return out


NAMES = ("ops", "aligned", "inserted", "confusion")


def mismatches(got, want) -> List[str]:
    """Exact: the names of the outputs that are not array_equal (shape included)."""
    return [n for n, a, b in zip(NAMES, got, want) if not np.array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64))]


def assert_identities(ops, aligned, inserted, idx, ln, tg, fallback: bool, distance):
    """The identities every clip satisfies; `distance(a, b)` is an independent Levenshtein distance."""
    T = idx.shape[1]
    for b in range(idx.shape[0]):
        a = prediction(idx[b], ln[b], T, fallback)
        t = [int(x) for x in tg[b]]
        t = t[:t.index(PAD)] if PAD in t else t
        m, s, d, i = (int(x) for x in ops[b])
        assert s + d + i == distance(a, t), b
        assert m + s + d == len(t) and m + s + i == len(a), b
        assert int(inserted[b].sum()) == i, b
        if all(x != -1 for x in a):
            assert int((aligned[b] == -1).sum()) == d, b
        assert (aligned[b, len(t):] == -2).all() and (inserted[b, len(t) + 1:] == 0).all(), b
