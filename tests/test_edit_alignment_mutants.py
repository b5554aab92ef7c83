"""CPU: the edit alignment restated in the arrangement of the kernel (csrc/score_align.hip) -- one lane per target position, the rows over
the prediction with the insertion chain as a prefix minimum, each row's moves as an up-mask and a left-mask decided from the three values a
lane holds, the walk on those masks one run of equal moves per step, ended at row 0 or column 0, the counts derived from the diagonal
moves -- with switchable mistakes.  Without a mistake it equals the host reference on every case of tests/test_edit_alignment_gpu.py; each
mistake changes an integer output on at least one of them, so the array_equal of the GPU test would catch it."""
import numpy as np
import pytest

import edit_alignment_parity as P
from ishara_amd.tflite_model import FALLBACK_PHRASE

MUTANTS = {
    "up_first": "up tried before diagonal",
    "left_first": "left tried before up",
    "swap_del_ins": "deletions and insertions swapped in ops",
    "trail_slot": "trailing insertions counted in slot nb-1",
    "aligned_pad0": "aligned padded with 0 instead of -2",
    "fallback_lt2": "the fallback applied at out_len < 2",
    "fallback_ignored": "the fallback flag ignored",
    "transposed": "the confusion matrix transposed",
    "no_drain": "the walk stopped at i == 0 without draining j",
}


def restate(idx, ln, tg, fallback, mut=()):
    """(ops, aligned, inserted, confusion) by the kernel's arrangement, the mistakes in `mut` switched on"""
    assert set(mut) <= set(MUTANTS), mut
    B, T = idx.shape
    L = tg.shape[1]
    ops, aligned, inserted = np.zeros((B, 4), np.int64), np.zeros((B, L), np.int64), np.zeros((B, L + 1), np.int64)
    conf = np.zeros((60, 60), np.int64)
    lane = np.arange(64)
    j = lane + 1
    for b in range(B):
        bj = np.full(64, 59, np.int64)
        bj[:L] = tg[b]
        pads = np.nonzero(bj == 59)[0]
        nb = int(pads[0]) if pads.size else 64
        na = min(max(int(ln[b]), 0), T)
        a = idx[b, :na].astype(np.int64)
        if fallback and "fallback_ignored" not in mut and na < (2 if "fallback_lt2" in mut else 3):
            a = np.asarray(FALLBACK_PHRASE, np.int64)
            na = a.shape[0]
        # forward: lane l holds D[i][l + 1]; a row's moves as two 64-bit masks
        p = j.copy()
        up_m, left_m = np.zeros((na, 64), bool), np.zeros((na, 64), bool)
        for i in range(1, na + 1):
            left = np.concatenate([[i - 1], p[:-1]])
            diag = left + (a[i - 1] != bj)
            v = np.minimum.accumulate(np.minimum(diag, p + 1) - j)
            pn = j + np.minimum(i, v)
            if "up_first" in mut:
                is_up = p + 1 == pn
                is_diag = ~is_up & (diag == pn)
                is_left = ~is_up & ~is_diag
            elif "left_first" in mut:
                is_diag = diag == pn
                is_left = ~is_diag & (np.concatenate([[i], pn[:-1]]) + 1 == pn)
                is_up = ~is_diag & ~is_left
            else:
                is_diag = diag == pn
                is_up = ~is_diag & (p + 1 == pn)
                is_left = ~is_diag & ~is_up
            up_m[i - 1], left_m[i - 1] = is_up, is_left
            p = pn
        # walk: a step takes a run of equal moves inside the 64-row chunk of row i (lane src - k holds row i - k); it stops at row 0 (the
        # target positions left are deletions: no row took them) or at column 0 (the rows left are insertions in slot 0)
        i, jj = na, nb
        ali, ins = np.zeros(64, np.int64), np.zeros(65, np.int64)
        ins_rows = []
        while i > 0 and jj > 0:
            src, bit, base = (i - 1) & 63, jj - 1, (i - 1) & ~63
            n = 1
            if up_m[i - 1, bit]:
                while n <= src and up_m[i - 1 - n, bit]:
                    n += 1
                ins[max(nb - 1, 0) if (jj == nb and "trail_slot" in mut) else jj] += n
                ins_rows += list(range(i - n + 1, i + 1))
                i -= n
            elif not left_m[i - 1, bit]:
                while n <= src and bit - n >= 0 and not up_m[i - 1 - n, bit - n] and not left_m[i - 1 - n, bit - n]:
                    n += 1
                for t in range(n):
                    ali[bit - t] = i - t
                i, jj = i - n, jj - n
            else:
                while bit - n >= 0 and left_m[i - 1, bit - n]:
                    n += 1
                jj -= n
            assert i >= base
        if i > 0:
            ins[max(nb - 1, 0) if (nb == 0 and "trail_slot" in mut) else 0] += i
            ins_rows += list(range(1, i + 1))
        undrained = jj if (i == 0 and "no_drain" in mut) else 0      # the mistake: these positions are left as if they did not exist
        mine = (lane < nb) & (lane >= undrained)
        hit = mine & (ali > 0)
        symb = np.where(hit, a[np.maximum(ali, 1) - 1] if na else -1, -1)
        for l in np.nonzero(mine)[0]:
            conf[P.sym(int(bj[l])), P.sym(int(symb[l])) if hit[l] else 59] += 1
        for r in ins_rows:
            conf[59, P.sym(int(a[r - 1]))] += 1
        n_diag, m = int(hit.sum()), int((hit & (symb == bj)).sum())
        n_del, n_ins = int(mine.sum()) - n_diag, na - n_diag
        ops[b] = (m, n_diag - m, n_ins, n_del) if "swap_del_ins" in mut else (m, n_diag - m, n_del, n_ins)
        aligned[b] = np.where(mine, np.where(hit, symb, -1), 0 if "aligned_pad0" in mut else -2)[:L]
        inserted[b] = ins[:L + 1]
    return ops, aligned, inserted, (conf.T.copy() if "transposed" in mut else conf)


RUNS = [(T, L, fb) for T, L in P.SHAPES for fb in (False, True)]


def test_the_restatement_equals_the_host_reference():
    for T, L, fb in RUNS:
        got = restate(*P.pack(P.cases(T, L), T, L), fb)
        assert not P.mismatches(got, P.reference(T, L, fb)), (T, L, fb, P.mismatches(got, P.reference(T, L, fb)))


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_each_mistake_changes_an_integer_output(mut):
    hit = [(T, L, fb) for T, L, fb in RUNS if P.mismatches(restate(*P.pack(P.cases(T, L), T, L), fb, (mut,)), P.reference(T, L, fb))]
    print(f"{mut} ({MUTANTS[mut]}): caught at (T, L, fallback) = {hit}")
    assert hit, f"{mut}: no case of the GPU test sees it"
