"""CPU: the bounds of tests/test_ctc_gpu.py reject ordinary mistakes of a CTC kernel.  Each mistake of ctc_parity.MUTANTS is switched on in
the fp64 restatement of the recursions on the cases the GPU test draws, the mutant's gradient is rounded to float32 as a kernel's would be and
compared with the clean oracle through the GPU test's own compare(): on at least one case a quantity must exceed its bound by 2x -- a kernel
making that mistake cannot pass.  Also: with nothing switched on the restatement is the oracle, and the closed form of a single-alignment
sample is the oracle."""
import numpy as np
import pytest

import ctc_parity as P

TIGHT_33, TIGHT_33_SEAM_REPEAT = P.TIGHT.index((33, ())), P.TIGHT.index((33, (32,)))
# mistake -> the cases it is looked for on, grad_scale
MUTANT_CASES = {
    "skip_equal": ([P.case_a(31), P.case_g()], 1.0),
    "a2_carry": ([P.case_c(TIGHT_33), P.case_a(32)], 1.0),                     # one alignment, stepping 63 -> 65
    "a1_carry": ([P.case_c(TIGHT_33_SEAM_REPEAT), P.case_a(63)], 1.0),         # one alignment, stepping 63 -> 64 -> 65
    "b2_carry": ([P.case_c(TIGHT_33), P.case_a(32)], 1.0),
    "b1_carry": ([P.case_c(TIGHT_33_SEAM_REPEAT), P.case_a(63)], 1.0),
    "final_no_sm2": ([P.case_a(31), P.case_b(8, 9)], 1.0),
    "S_full": ([P.case_a(31), P.case_b(8, 17)], 1.0),
    "empty_init1": ([P.case_b(8, 9), P.case_b(8, 1)], 1.0),
    "em_prev": ([P.case_b(8, 9)], 1.0),
    "skip_group_last": ([P.case_b(8, 9), P.case_b(64, 17)], 1.0),
    "blank_last": ([P.case_e(60, 0), P.case_e(5, 0)], 1.0),
    "no_div_p": ([P.case_b(8, 9)], 1.0),
    "scale_post_only": ([P.case_g()], 0.25),
}
assert set(MUTANT_CASES) == set(P.MUTANTS)

CLEAN = [P.case_a(31), P.case_a(64), P.case_b(8, 1), P.case_b(8, 9), P.case_b(64, 33), P.case_c(TIGHT_33), P.case_c(TIGHT_33_SEAM_REPEAT),
         P.case_e(5, 0), P.case_e(60, 30), P.case_e(2, 0), P.case_f(64, 96, "n12"), P.case_f(64, 96, "trained"), P.case_g()]


@pytest.mark.parametrize("case", CLEAN, ids=lambda c: c.name)
def test_unmutated_restatement_is_the_oracle(case):
    nll, grad = P.restate(P.logits(case), P.labels(case), case.blank)
    rn, rg = P.reference(case)
    ok = P.feasible(case)
    assert ok.any()
    assert np.allclose(nll[ok], rn[ok], rtol=1e-9, atol=1e-9)
    assert np.allclose(grad[ok], rg[ok], rtol=1e-9, atol=1e-9)
    assert (nll[~ok] >= P.SENTINEL).all() and (rn[~ok] >= P.SENTINEL).all()
    obs, bad = P.compare(case, nll, grad)
    assert not bad and max(obs.values()) < 1e-3, obs


@pytest.mark.parametrize("i", range(len(P.TIGHT)), ids=lambda i: "len%d-rep%d" % (P.TIGHT[i][0], len(P.TIGHT[i][1])))
def test_closed_form_of_one_alignment_is_the_oracle(i):
    case = P.case_c(i)
    nll, grad = P.closed_form(case)
    rn, rg = P.reference(case)
    assert np.allclose(nll, rn, rtol=1e-12, atol=1e-9) and np.allclose(grad, rg, rtol=0, atol=1e-9)


def test_the_seam_cases_sit_on_the_seams():
    """what the builder promises: lattice ends at 64k-1, 64k+1, 64k+3; labels 32k-1 and 32k equal in one copy and different in the other"""
    case = P.case_a(255)
    y, (n, rep) = P.labels(case), P.lengths(case)
    assert {int(2 * v + 1) for v in n} >= {64 * k + d for k in range(1, 8) for d in (-1, 1, 3)} | {1, 3, 511}
    assert rep.max() <= 6 and P.feasible(case).all()
    for k in range(1, 8):
        same = {bool(y[b, 32 * k - 1] == y[b, 32 * k]) for b in range(case.B) if n[b] == 32 * k + 1}
        assert same == {True, False}, k
    for L, ns in zip(P.A_LS, P.A_NS):
        assert (2 * L + 1 + 63) // 64 == ns


@pytest.mark.parametrize("mut", sorted(P.MUTANTS))
def test_bounds_reject_the_mutant(mut):
    cases, gs = MUTANT_CASES[mut]
    worst = {}
    for case in cases:
        nll, grad = P.restate(P.logits(case), P.labels(case), case.blank, gs, mut=(mut,))
        obs, _ = P.compare(case, nll.astype(np.float32), grad.astype(np.float32), gs)
        worst[case.name] = max(obs.values())
    print(f"{mut} ({P.MUTANTS[mut]}): worst err / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) >= 2.0, f"{mut}: no case exceeds 2x a bound: {worst}"
