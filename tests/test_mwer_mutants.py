"""CPU: the checks of tests/mwer_parity.py can fail.  The numpy twins of ishara_ctc_nbest_grad and ishara_mwer_weights pass them as they
are; with one mistake switched on each falls outside the bound (or loses the bit-equality the check asks for) on at least one case."""
import numpy as np
import pytest

import mwer_parity as P


def test_the_unmutated_twins_pass():
    worst = 0.0
    for case in P.grad_cases():
        fails, ratio = P.check_grad(case, P.twin_grad(case).astype(np.float32))
        assert not fails, fails
        worst = max(worst, ratio)
    print(f"twin_grad in float32 storage: worst err / bound {worst:.3g}")
    for case in P.weight_cases():
        fails, ratio = P.check_weights(case, P.twin_weights(case))
        assert not fails, fails


@pytest.mark.parametrize("mutant", P.GRAD_MUTANTS)
def test_gradient_mutants_are_caught(mutant):
    caught = []
    for case in P.grad_cases():
        with np.errstate(all="ignore"):
            fails, ratio = P.check_grad(case, P.twin_grad(case, mutant).astype(np.float32))
        if fails:
            caught.append((case["name"], ratio))
    print(f"{mutant}: caught on {len(caught)} of {len(P.grad_cases())} cases, e.g. {caught[:3]}")
    assert caught, f"the mistake '{mutant}' passes every case"


def test_only_a_row_that_does_not_sum_to_zero_exposes_a_dropped_softmax_term():
    """sum_n coef_n * softmax vanishes with the row's sum: the tables need a row that does not sum to 0, and have one that does"""
    sums = np.concatenate([np.where(P.participating(c), c["coef"], 0).sum(axis=1) for c in P.grad_cases()])
    assert (np.abs(sums) < 1e-6).any() and (np.abs(sums) > 0.5).any()
    zeros = np.concatenate([c["coef"].ravel() for c in P.grad_cases()])
    assert (zeros == 0).any() and np.signbit(zeros[zeros == 0]).any() and (zeros > 0).any() and (zeros < 0).any()


@pytest.mark.parametrize("mutant", P.WEIGHT_MUTANTS)
def test_weight_mutants_are_caught(mutant):
    caught = []
    for case in P.weight_cases():
        fails, _ = P.check_weights(case, P.twin_weights(case, mutant))
        if fails:
            caught.append(case["name"])
    print(f"{mutant}: caught on {caught}")
    assert caught, f"the mistake '{mutant}' passes every case"
