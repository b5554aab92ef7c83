"""CPU: the bound of tests/ensemble_parity.py is tight enough to tell a right ishara_logits_combine from a wrong one.  The float32 twin of
the kernel passes every case of the table; each of nine mistakes a kernel of this kind can make is rejected by at least one case.  The
constant of the bound comes from here as well: K_HOST is the unmutated twin's worst err / (2^-24 * scale), K = 4 * K_HOST."""
import pytest

import ensemble_parity as P


def test_the_twin_passes_every_case_and_k_host_is_what_was_measured():
    k_host = P.measure_k_host()
    print(f"K_host measured {k_host:.3f}, recorded {P.K_HOST}, K = {P.K}")
    # numpy's float32 exp / log differ by an ulp between its SIMD builds, which moves the worst case a little: the recorded constant must
    # stay what such a measurement gives, not become a free parameter
    assert P.K_HOST / 2 <= k_host <= 2 * P.K_HOST, "the recorded K_HOST is not what the fp32 twin measures on this host"
    assert P.K == 4 * P.K_HOST
    for c in P.cases():
        assert P.compare(c, P.twin(c)) <= 1, c["name"]


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_the_bound_rejects_the_mistake(mutant):
    ratios = {c["name"]: P.compare(c, P.twin(c, mutant)) for c in P.cases()}
    caught = [n for n, r in ratios.items() if r > 1]
    print(f"{mutant}: rejected by {len(caught)} of {len(ratios)} cases, smallest rejecting err / bound {min(ratios[n] for n in caught) if caught else None}")
    assert caught, f"{mutant}: no case of the table rejects it"
    assert all(ratios[n] > 10 for n in caught), f"{mutant}: a rejection within a factor 10 of the bound is luck, not a test"
