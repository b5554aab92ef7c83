"""CPU: the checks of tests/kd_parity.py are tight enough to tell a right ishara_kd_grad from a wrong one.  Each of eight mistakes a kernel of
this kind can make is rejected by at least one case of the table: by the gradient bound, the KL bound, the rule for rows past a clip's end,
or the exact bf16 copy.  The constants of the bounds come from the unmutated twin (tests/test_kd.py measures them)."""
import numpy as np
import pytest

import kd_parity as P


def _verdict(c, mutant):
    """the largest err / bound over the four checks a GPU run goes through: accumulate 0 and 1, kl_frame, and dlb (inf when it is not exact)"""
    o = P.old_rows(c)
    t, ta = P.twin(c, mutant), P.twin(c, mutant, old=o)
    r = max(P.compare_grad(c, t["dlogits"]), P.compare_kl(c, t["kl_frame"]), P.compare_grad(c, ta["dlogits"], old=o))
    if not (np.array_equal(t["dlb"], P.dlb_of(t["dlogits"])) and np.array_equal(ta["dlb"], P.dlb_of(ta["dlogits"]))):
        r = float("inf")
    return r


def test_k_host_is_printed():
    kg, kk = P.measure_k_host()
    print(f"K_HOST measured {kg:.3f} (recorded {P.K_HOST}), K_HOST_KL measured {kk:.3f} (recorded {P.K_HOST_KL})")
    assert kg <= P.K_HOST and kk <= P.K_HOST_KL


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_the_checks_reject_the_mistake(mutant):
    ratios = {c["name"]: _verdict(c, mutant) for c in P.cases()}
    caught = [n for n, r in ratios.items() if r > 1]
    print(f"{mutant}: rejected by {len(caught)} of {len(ratios)} cases, smallest rejecting err / bound {min(ratios[n] for n in caught) if caught else None}")
    assert caught, f"{mutant}: no case of the table rejects it"
    assert all(ratios[n] > 10 for n in caught), f"{mutant}: a rejection within a factor 10 of the bound is luck, not a test"
