"""CPU: the checks of tests/mbr_parity.py have teeth.  The float32 twin of ishara_mbr_select passes every case; each of the mistakes a
bit-vector edit distance, a vote or a risk sum invites is rejected by at least one case, the vote mistake by more than 10 x its bound."""
import numpy as np
import pytest

import mbr_parity as P


def test_the_twin_passes_and_k_host_is_what_was_measured():
    worst = 0.0
    for c in P.cases():
        fails, ratio = P.check(c, P.twin(c))
        assert not fails, (c["name"], fails[:3])
        worst = max(worst, ratio)
    k_host = P.measure_k_host()
    print(f"float32 twin: worst w_out err / bound {worst:.3f} at K = {P.K}; measured K_HOST {k_host:.3f} (recorded {P.K_HOST})")
    assert k_host <= P.K_HOST, f"K_HOST {P.K_HOST} is below the twin's own error {k_host}"
    assert P.K == 4 * P.K_HOST


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_mutant_is_rejected(mutant):
    rejected = {}
    for c in P.cases():
        fails, ratio = P.check(c, P.twin(c, mutant))
        if fails:
            rejected[c["name"]] = (fails[0], ratio)
    print(f"{mutant}: rejected by {len(rejected)} of {len(P.cases())} cases, e.g. {next(iter(rejected.items()), None)}")
    assert rejected, f"no case rejects {mutant}"
    if mutant == "unshifted_scores":                      # the only mistake that lands in the toleranced item: far outside, not at its edge
        assert max(r for _, r in rejected.values()) > 10.0


def test_a_vote_ten_bounds_off_is_rejected():
    """the toleranced item itself: a vote moved by 10 x its bound fails, one moved by half its bound passes"""
    c = next(c for c in P.cases() if c["weights"] is None and c["N"] == 31)
    ref, x = P.votes64(c["name"])
    base = P.twin(c)
    b, n = np.argwhere((ref > 0) & (x < 0))[0]
    for factor, passes in ((10.0, False), (0.4, True)):
        got = {k: v.copy() for k, v in base.items()}
        got["w_out"][b, n] = np.float32(ref[b, n] * (1.0 + factor * (2.0 * abs(x[b, n]) + P.K) * P.EPS))
        # risk and best follow the moved vote: recompute them so that only item 3 is in question
        from ishara_amd import mbr
        best, risk, _, _ = mbr.mbr_reference(P.case_lists(c)[b], mode=c["mode"], C=c["C"], votes=got["w_out"][b])
        got["risk"][b], got["best"][b] = risk, best
        lst = P.case_lists(c)[b][best]
        got["out_idx"][b] = -1
        got["out_idx"][b, :len(lst)] = lst
        got["out_len"][b] = len(lst)
        fails, ratio = P.check(c, got)
        assert (not fails) == passes, (factor, ratio, fails[:2])
