"""CPU: the forced-alignment recursion restated in the arrangement of the kernel (csrc/ctc_align.hip) -- state s = lane + 64 k, the s-1 / s-2
neighbours by lane rotations with the k-1 carry at lanes 0 and 1, the 2-bit back-pointers of a lane's states packed into one 16-bit word per
frame, the backtrace reading lane s % 64's word -- with switchable mistakes.  Without a mistake it equals the host reference on every case of
tests/test_ctc_align_gpu.py; each mistake changes an integer output on at least one of them, so the == of the GPU test would catch it."""
import numpy as np
import pytest

import ctc_parity as P
from ishara_amd.ctc_align import viterbi_align

MUTANTS = {
    "s2_carry": "the s-2 carry dropped for states s mod 64 in {0, 1}",
    "s1_carry": "the s-1 carry dropped at s mod 64 = 0",
    "skip_equal": "the s-2 transition allowed between equal labels",
    "end_tie": "the end chosen as S-2 on a tie",
    "s1_first": "s-1 preferred over stay on a tie",
    "bp_shift": "the back-pointer of register k read at bit k instead of bit 2 k",
}


def restate(x, y, blank, mut=()):
    """(frame_pos [B,T], start [B,L], end [B,L]) int32 by the kernel's arrangement, the mistakes in `mut` switched on"""
    assert set(mut) <= set(MUTANTS), mut
    x, y = np.asarray(x, np.float32), np.asarray(y, np.int64)
    B, T, Cc = x.shape
    L = y.shape[1]
    NS = (2 * L + 1 + 63) // 64
    fpos, start, end = np.full((B, T), -1, np.int32), np.full((B, L), -1, np.int32), np.full((B, L), -1, np.int32)
    lane, k = np.arange(64)[None, :], np.arange(NS)[:, None]
    s = lane + 64 * k                                                     # [NS, 64]
    dead = -np.inf
    for b in range(B):
        isb = np.nonzero(y[b] == blank)[0]
        n = int(isb[0]) if isb.size else L
        lab = y[b, :n]
        if ((lab < 0) | (lab >= Cc)).any() or T < n + int((lab[1:] == lab[:-1]).sum()):
            continue
        S = 2 * n + 1
        ext = np.full(64 * NS, blank, np.int64)
        ext[1:2 * n:2] = lab
        my = ext.reshape(NS, 64)
        act = s < S
        ext2 = np.concatenate([[blank, blank], ext[:-2]]).reshape(NS, 64)
        skp = act & (s >= 2) & (my != blank) & ((my != ext2) | ("skip_equal" in mut))
        v = np.where(act & ((s == 0) | ((s == 1) & (n > 0))), x[b, 0][my].astype(np.float64), dead)
        words = np.zeros((T, 64), np.uint16)
        for t in range(1, T):
            r1, r2 = np.roll(v, 1, axis=1), np.roll(v, 2, axis=1)         # lane l holds lane l-1 / l-2 of its own register
            up1 = np.concatenate([np.full((1, 64), dead), r1[:-1]])      # the same rotation of register k-1
            up2 = np.concatenate([np.full((1, 64), dead), r2[:-1]])
            a1 = np.where(lane >= 1, r1, dead if "s1_carry" in mut else up1)
            a2 = np.where(lane >= 2, r2, dead if "s2_carry" in mut else up2)
            p2 = np.where(skp, a2, dead)
            if "s1_first" in mut:
                best, back = a1, np.ones((NS, 64), np.uint16)
                m = v > best
                best, back = np.where(m, v, best), np.where(m, 0, back).astype(np.uint16)
            else:
                best, back = v, np.zeros((NS, 64), np.uint16)
                m = a1 > best
                best, back = np.where(m, a1, best), np.where(m, 1, back).astype(np.uint16)
            m = p2 > best
            best, back = np.where(m, p2, best), np.where(m, 2, back).astype(np.uint16)
            v = np.where(act, best + x[b, t][my].astype(np.float64), dead)
            words[t] = np.bitwise_or.reduce(back << (2 * k).astype(np.uint16), axis=0)
        flat = v.reshape(-1)
        st = S - 1
        if n > 0 and (flat[S - 2] >= flat[S - 1] if "end_tie" in mut else flat[S - 2] > flat[S - 1]):
            st = S - 2
        for t in range(T - 1, -1, -1):
            fpos[b, t] = st >> 1 if st & 1 else -1
            if t > 0:
                shift = (st >> 6) if "bp_shift" in mut else 2 * (st >> 6)
                st = max(st - ((int(words[t, st & 63]) >> shift) & 3), 0)
        f = fpos[b]
        for t in np.nonzero(f >= 0)[0]:
            i = min(int(f[t]), n - 1)
            if t == 0 or f[t - 1] != i:
                start[b, i] = t
            if t == T - 1 or f[t + 1] != i:
                end[b, i] = t + 1
    return fpos, start, end


TIES = P.Case("ties", 80, 60, 33, 59, ((33, ()), (33, (32,)), (20, (5,)), (1, ()), (0, ())), seed=1100)


def _inputs():
    """(name, logits, labels, blank) of cases the GPU test launches: seams, single alignments, regimes, the tie inputs"""
    cases = ([P.case_a(L) for L in (31, 32, 63, 64)] + [P.case_b(64, T) for T in (1, 9, 17)] + [P.case_c(i) for i in range(len(P.TIGHT))]
             + [P.case_d(5), P.case_e(2, 1), P.case_e(64, 0), P.case_f(64, 96, "flat"), P.case_f(64, 96, "trained"), P.case_g(), P.case_k(60, 63, 0)])
    out = [(c.name, P.logits(c), P.labels(c), c.blank) for c in cases]
    out.append(("ties-zero", np.zeros((TIES.B, TIES.T, TIES.C), np.float32), P.labels(TIES), TIES.blank))
    out.append(("ties-integer", np.round(P.logits(TIES)), P.labels(TIES), TIES.blank))
    return out


def _differs(a, b):
    return any(not np.array_equal(p, q) for p, q in zip(a[:3], b[:3]))


def test_the_restatement_equals_the_host_reference():
    for name, x, y, blank in _inputs():
        assert not _differs(restate(x, y, blank), viterbi_align(x, y, blank)), name


@pytest.mark.parametrize("mut", sorted(MUTANTS))
def test_each_mistake_changes_an_integer_output(mut):
    hit = [name for name, x, y, blank in _inputs() if _differs(restate(x, y, blank, (mut,)), viterbi_align(x, y, blank))]
    print(f"{mut} ({MUTANTS[mut]}): caught by {hit}")
    assert hit, f"{mut}: no case of the GPU test sees it"
