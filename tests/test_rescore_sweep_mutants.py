"""CPU: the cases of tests/rescore_sweep_parity.py reject ordinary mistakes.  twin_sweep restates csrc/rescore_sweep.hip in numpy (pairwise
dedupe, one float32 LM walk per slot, the 64-bit Myers word with the target as the pattern, max-then-lowest-slot selection); unmutated it
equals rescore_sweep_reference on every case with either fallback, and each mutant differs from it on at least one."""
import numpy as np
import pytest

import rescore_sweep_parity as SP


@pytest.mark.parametrize("fallback", [0, 1])
def test_the_twin_equals_the_reference(fallback):
    for case in SP.cases():
        got = SP.twin_sweep(case, fallback)
        assert not SP.compare(case, fallback, got), (case["name"], SP.compare(case, fallback, got))


def test_the_myers_word_reaches_bit_63():
    g = np.random.default_rng(3)
    t = g.integers(0, 5, 64).tolist()
    assert SP.myers(t, t) == 0 and SP.myers(t, t[:63]) == 1 and SP.myers(t, t + [7] * 6) == 6 and SP.myers(t, []) == 64 and SP.myers([], t) == 64


@pytest.mark.parametrize("mutant", SP.SWEEP_MUTANTS)
def test_every_mutant_is_rejected(mutant):
    caught = []
    for case in SP.cases():
        for fallback in (0, 1):
            if SP.compare(case, fallback, SP.twin_sweep(case, fallback, mutant)):
                caught.append((case["name"], fallback))
    print(f"{mutant}: rejected by {len(caught)} case runs, first {caught[:3]}")
    assert caught, f"no case rejects the mutant {mutant}"
